/*
 * ihgnn_hip.h - C ABI of libihgnn_hip.so: the MI355X (gfx950) hypergraph message-passing path of IHGNN.
 *
 * This is the drop-in boundary.  The reference reaches this path through PyTorch
 * modules plus one third-party operator (torch_sparse.matmul); each entry point below names the
 * reference interface it replaces (paths relative to the CDboyOne/IHGNN checkout).
 *
 * Conventions for every device entry point:
 *   - plain pointers and sizes only; all device buffers are caller-owned, row-major fp32 / int32;
 *   - `ld_*` is the row stride in ELEMENTS (lets a layer read/write a column slice of the [N, D] feature
 *     matrix in place);
 *   - `stream` is a hipStream_t passed as void*; kernels are enqueued on it and the call returns at once:
 *     no allocation, no synchronisation, no host<->device copies (graph-capturable);
 *   - return value: 0 on success, negative IHG_ERR_* otherwise; ihg_last_error_string() describes the
 *     last failure on the calling thread.
 *   - Rows whose base address and stride are 16-byte aligned with dim % 4 == 0 take the 16-B/lane path;
 *     anything else is still computed (4-B/lane path), never rejected.
 */
#ifndef IHGNN_HIP_H
#define IHGNN_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define IHG_OK                0
#define IHG_ERR_INVALID      -1   /* bad argument (null pointer, negative size, unsupported order, ...) */
#define IHG_ERR_LAUNCH       -2   /* HIP runtime reported an error at launch */
#define IHG_ERR_WORKSPACE    -3   /* caller-provided workspace too small */

#define IHG_SCALE_NONE        0
#define IHG_SCALE_MULTIPLY    1   /* out[r] = scale[r] * sum   (Dv^-1, Dv^-1/2) */
#define IHG_SCALE_DIVIDE      2   /* out[r] = sum / scale[r]   (EmbeddingBag 'mean': scale = bag length) */
#define IHG_SRC_READ_ONCE     0x400 /* OR-ed into out_scale_mode of ihg_node_segment_sum: every source row is read exactly once by this launch (a scatter of per-member rows) - non-temporal loads */
#define IHG_SCALE_ACCUMULATE  0x100 /* OR-ed into out_scale_mode of ihg_node_segment_sum: out[r] += (scaled) sum - the hyperedge chunks of one scatter add up in `out` */
#define IHG_SRC_SCALE_IN_ENTRIES 0x800 /* OR-ed into out_scale_mode of ihg_node_segment_sum: entry_scale[k] already holds src_scale[ids[k]] (times the entry's own weight), so the gather does not fetch src_scale per id; src_scale is still read for the row's own term (self_weight).  Needs both pointers. */

typedef void* ihg_stream_t;       /* hipStream_t */

/* Version of this ABI; bumped on any signature change. */
int32_t ihg_abi_version(void);

/* 1 when the library was built with an ablation switch of csrc/ablate.hpp (tools/ab_variant.sh ... -DIHG_ABL_*: a kernel with one class of its work removed, wrong
 * results on purpose, for timing only); the product build returns 0 and the binding refuses anything else unless IHG_ALLOW_ABLATION_BUILD=1. */
int32_t ihg_ablation_build(void);

/* Text of the last error raised on this thread ("" if none). */
const char* ihg_last_error_string(void);

/* ------------------------------------------------------------------------------------------------
 * HOST: hypergraph incidence layout.   Replaces PpsHyperGraph.from_interactions
 * (Helpers/Graph.py:94-134) and torch_sparse's SparseTensor...coalesce() (Models/GnnLayers.py:190).
 *
 * triples[e] = (user, query, item), 0-based per type, in file order (one hyperedge per positive
 * interaction; duplicates stay distinct).  Outputs, all host buffers sized by the caller:
 *   i3       [E,3]  global node ids  u, q+U, i+U+Q                     (Graph.py:110-111,117,129)
 *   rowptr   [N+1]  node-major CSR offsets; edge_ids [3E] hyperedge ids, ascending inside a node
 *                   (= the coalesced COO order of Graph.py:123-128)
 *   degree   [N]    incident hyperedges, 0 replaced by 1e-8             (Graph.py:112,120)
 * Returns IHG_ERR_INVALID if a triple is out of range.
 */
int ihg_build_csr(const int64_t* triples, int64_t n_edges,
                  int64_t n_users, int64_t n_queries, int64_t n_items,
                  int32_t* i3, int32_t* rowptr, int32_t* edge_ids, float* degree);

/* HOST: search-log CSV ingestion.  Replaces SearchLogCollection.read + SearchLog.parse + the positive / negative split
 * of GraphDataset.__init__ (Helpers/SearchLogCollection.py:25-32, Helpers/SearchLog.py:63-71, Dataset.py:195-213) for the
 * quantities the graph needs.  File: one header line, then rows `user,query,search_time,items,pages,positions,
 * interactions,times` whose list fields are space-separated; item k of a row is a positive interaction when
 * interactions[k] > 0.  Pass pos == neg == NULL to count (n_logs / n_pos / n_neg), then call again with buffers of
 * [n_pos,3] / [n_neg,3] int64 to receive the (user, query, item) triples in file order.  neg may stay NULL.
 * pos_log (may be NULL; [n_pos] int64): the 0-based row of each positive - rows with several positives are the
 * variable-arity hyperedges of ihg_build_log_hypergraph.
 */
int ihg_parse_search_logs(const char* path, int64_t* n_logs, int64_t* n_pos, int64_t* n_neg,
                          int64_t* pos, int64_t pos_capacity, int64_t* neg, int64_t neg_capacity, int64_t* pos_log);

/* HOST: `graph_info.txt` (one line "users queries items vocabulary", Dataset.py:143-147) -> counts[4]. */
int ihg_read_graph_info(const char* path, int64_t* counts);

/* HOST: `queries_multihot.txt` (line r = space-separated 0-based word ids of query r, Dataset.py:165-176; an empty line is a
 * query without words).  Two-pass like the CSV parser: offsets == words == NULL counts; then offsets[n_queries] = start of each
 * query's words in words[n_words] (the nn.EmbeddingBag input / offsets of Dataset.py:161-186, before the +1 padding shift).
 */
int ihg_read_query_bags(const char* path, int64_t* n_queries, int64_t* n_words, int64_t* offsets, int64_t offsets_capacity,
                        int64_t* words, int64_t words_capacity);

/* HOST: per-search-log hypergraph.  Replaces PpsLogHyperGraph.from_search_logs (Helpers/Graph.py:138-189): one hyperedge of
 * VARIABLE arity per search log with >= 1 positive, members [user, query + U, positive items + U + Q].  Input: the positives
 * and their row numbers as ihg_parse_search_logs returns them (positives of one log consecutive).  Output, caller-sized
 * (n_edges <= n_pos, nnz <= 3 n_pos): the incidence in BOTH orientations as CSR with values -
 *   edge_ptr [n_edges+1], edge_nodes / edge_vals [nnz]   edge-major (members ascending; a repeated item is one entry of value 2,
 *                                                        as coalesce() sums duplicates, Graph.py:178-184)
 *   node_ptr [N+1], node_edges / node_vals [nnz]         node-major, hyperedge ids ascending (= the coalesced COO order)
 *   edge_degree [n_edges] = len(members) with repeats (Graph.py:167), node_degree [N] = hyperedges containing the node, 0 -> 1e-8
 *   (Graph.py:166,171).
 */
int ihg_build_log_hypergraph(const int64_t* pos, const int64_t* pos_log, int64_t n_pos, int64_t n_users, int64_t n_queries, int64_t n_items,
                             int32_t* edge_ptr, int32_t* edge_nodes, float* edge_vals, float* edge_degree, int32_t* node_ptr,
                             int32_t* node_edges, float* node_vals, float* node_degree, int64_t* n_edges_out, int64_t* nnz_out);

/* HOST: pairwise graph of the GCN baseline.  Replaces Pps2DGraph.from_interactions (Helpers/Graph.py:19-81) and the
 * coalesce() of its adjacency.  completeness: 0 = uqi (u-q, q-i, i-u per interaction), 1 = uq, 2 = ui, 3 = qi
 * (Graph.py:40-63; every pair is stored in both directions).  Output: CSR of the symmetric [N x N] adjacency with
 * duplicate pairs SUMMED into `vals`, `degree` = entries per node before coalescing (+1 with self loops), 0 -> 1e-8
 * without self loops (Graph.py:68-69).  `cols`/`vals` must hold `capacity` >= 6E (+N) entries; *nnz_out = entries used.
 */
int ihg_build_pair_csr(const int64_t* triples, int64_t n_edges, int64_t n_users, int64_t n_queries, int64_t n_items,
                       int32_t completeness, int32_t self_loops,
                       int32_t* rowptr, int32_t* cols, float* vals, float* degree, int64_t capacity, int64_t* nnz_out);

/* HOST: merge the repeated ids of every row of a CSR: row r of (out_ptr, out_ids, out_counts) holds the DISTINCT ids of row r of (ptr, ids) in ascending
 * order with their multiplicities as floats (exact: a count) - or, with `weights` (one float per input id), the SUM of the weights of each distinct id.
 * Applied to the two-hop list of the hypergraph (node -> the other two members of each of
 * its hyperedges, Helpers/Graph.py:107-118 composed with itself as Models/GnnLayers.py:233-234 does through two SpMMs) it gives H H^T - diag(deg) as a
 * weighted CSR: a (user, query) pair that co-occurs in k hyperedges is ONE entry of weight k instead of k gathers (duplicate hyperedges stay distinct
 * hyperedges: the multiplicities carry them).  out_ids / out_counts hold ptr[n_rows] entries; *nnz_out = entries used.  out_ids == NULL: count only
 * (out_ptr and *nnz_out are written).
 */
int ihg_merge_id_lists(const int32_t* ptr, const int32_t* ids, const float* weights, int64_t n_rows, int32_t* out_ptr, int32_t* out_ids, float* out_counts,
                       int64_t* nnz_out);

/* HOST: the DISTINCT (user, query, item) triples of `triples` [n_edges, 3] (0-based per type, as ihg_build_csr takes them), ascending by (user, query, item), with
 * how often each occurs.  The reference makes one hyperedge per positive interaction, duplicates included (Helpers/Graph.py:107-118); every quantity the
 * path computes from duplicates - vertex degrees, H Ef, H^T of a cotangent - is the distinct hyperedge's value times its multiplicity, so a layout may keep each triple
 * once and carry count_out as a per-hyperedge weight (IncidenceLayout.edge_weight): same results, a fraction of the rows on search logs that repeat.
 *   unique_out [n_edges, 3] (capacity), count_out [n_edges], file_to_unique [n_edges] (optional: index of the distinct triple of every input row);
 *   *n_unique_out = distinct triples.  unique_out == NULL: count only.
 */
int ihg_unique_triples(const int64_t* triples, int64_t n_edges, int64_t n_users, int64_t n_queries, int64_t n_items,
                       int64_t* unique_out, float* count_out, int32_t* file_to_unique, int64_t* n_unique_out);

/* HOST: invert any CSR (row -> sorted list of column ids) into its transpose.  Used for the
 * EmbeddingBag backward (word -> bags containing it).  Replaces the autograd-generated
 * _embedding_bag_dense_backward of Models/EmbeddingLayers.py:79.
 *   ptr [n_rows+1], ids [nnz]  ->  t_ptr [n_cols+1], t_rows [nnz] (ascending row inside a column)
 */
int ihg_transpose_csr(const int32_t* ptr, const int32_t* ids, int64_t n_rows, int64_t n_cols,
                      int32_t* t_ptr, int32_t* t_rows);

/* ------------------------------------------------------------------------------------------------
 * DEVICE: node -> hyperedge gather-sum (K5, first-order / HGCN form).
 *   out[e,:] = alpha * ( s(i3[e,0])*src[i3[e,0],:] + s(i3[e,1])*src[i3[e,1],:] + s(i3[e,2])*src[i3[e,2],:] ) + bias
 * with s(v) = node_scale[v] (or 1 if node_scale == NULL) and bias optional [dim].
 * Replaces: node_features[I3] gather + Linear of FeatureInteractor order 1 (Models/CommonLayers.py:60-66,
 * after hoisting the Linear to node level), thsp.matmul(incidence_t, x) * De^-1 of HGCNLayer
 * (Models/GnnLayers.py:148-149), and the autograd backward of thsp.matmul(incidence, .) (GnnLayers.py:233).
 * edge_scale (optional, [n_edges]): the sum of hyperedge e is multiplied by alpha * edge_scale[e] - a layout that keeps each DISTINCT (user, query, item) triple once
 * passes the triple's multiplicity here where the result is the cotangent of all its copies (the backward of the hyperedge -> node pass; duplicates are distinct
 * hyperedges in the reference, Helpers/Graph.py:107-118, and m identical rows of H sum to m times one of them).
 */
int ihg_edge_gather_sum(const float* src, int64_t ld_src, const int32_t* i3,
                        const float* node_scale, const float* bias, float alpha, const float* edge_scale,
                        float* out, int64_t ld_out, int64_t n_edges, int32_t dim, ihg_stream_t stream);

/* The same sum (alpha = 1, no bias) written as the member-gradient kernel's operand instead of fp32 rows (the backward of thsp.matmul(incidence, .), GnnLayers.py:233, whose
 * result only ihg_interact_bwd_user_reduced_planes reads): row e of `planes` is [2][dim] fp16 - the row scaled by the power of two that brings its largest magnitude
 * to [2^13, 2^14), as hi = fp16(x) and lo = fp16(x - hi) - and inv_scale[e] the inverse of that power.  4 dim bytes per row, like the fp32 row.  dim 256
 * (ihg_edge_gather_sum_planes_supported).  edge_scale: as in ihg_edge_gather_sum (applied before the row is scaled and split).
 */
int32_t ihg_edge_gather_sum_planes_supported(int32_t dim, int64_t ld_src);
int ihg_edge_gather_sum_planes(const float* src, int64_t ld_src, const int32_t* i3, const float* node_scale, const float* edge_scale,
                               void* planes, float* inv_scale, int64_t n_edges, int32_t dim, ihg_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * DEVICE: hyperedge -> node segment-sum (K7 + K8).
 *   out[r,:] = scale_op( sum_{k in [rowptr[r], rowptr[r+1])} w(ids[k]) * src[ids[k],:] , out_scale[r] )
 * with w(ids[k]) = src_scale[ids[k]] (or 1), times entry_scale[k] when given (values of a weighted CSR: the pairwise
 * adjacency of GCNLayer, Models/GnnLayers.py:37-41).  Rows longer than `heavy_threshold` entries go through the split-row plan below
 * (pass n_heavy = 0 to sum every row with a single lane group).
 * `self_weight` (optional, [n_rows], only for square operators whose ids index the same table as the output rows) adds
 * self_weight[r] * w(r) * src[r,:] to row r before the output scale: the diagonal of a two-hop (node -> hyperedge -> node)
 * operator, whose off-diagonal part is then listed without the row's own id.
 * `row_order` (optional, [n_rows]) is the order in which rows are handed to lane groups - a permutation sorted by
 * decreasing row length keeps the groups of one wave equally busy; NULL = natural order.  Results do not depend on it.
 * It may also be a SUBSET of the rows (n_rows = its length; rowptr is still indexed by row id): only those rows, and the
 * rows of the split-row plan, are written - the last layer of a training step, whose output is read at the batch rows only.
 * With IHG_SRC_SCALE_IN_ENTRIES in the mode word w(ids[k]) = entry_scale[k] alone: the caller has folded src_scale[ids[k]] into the entries (a list and a scale
 * vector that stay the same from launch to launch: one coalesced 4-byte load beside the id instead of a divergent gather per id); w(r) of the row's own term stays src_scale[r].
 * `src_mask` (optional, one byte per source row): rows with a 0 are known to be all-zero and are not fetched (the gradient
 * of that last layer's output is zero outside the batch rows).
 * Replaces: thsp.matmul(self.incidence, edge_features) and Dv^-1 * / Dv^-1/2 * (Models/GnnLayers.py:151-152,
 * 233-234), nn.EmbeddingBag(mode='mean') (Models/EmbeddingLayers.py:79, via ihg_bag_mean_fwd), and the
 * index_put(accumulate) backward of the three row gathers (Models/CommonLayers.py:70-72).
 */
int ihg_node_segment_sum(const float* src, int64_t ld_src, const int32_t* rowptr, const int32_t* ids,
                         const int32_t* row_order,
                         const float* src_scale, const float* entry_scale,
                         const float* out_scale, int32_t out_scale_mode,
                         float* out, int64_t ld_out, int64_t n_rows, int32_t dim,
                         int32_t heavy_threshold,
                         const int32_t* seg_begin, const int32_t* seg_end, int64_t n_segments,
                         const int32_t* heavy_rows, const int32_t* heavy_segptr, int64_t n_heavy,
                         float* partials, const float* self_weight, const uint8_t* src_mask, ihg_stream_t stream);
/* Split rows (skewed / power-law degree distributions): the host cuts every row longer than `heavy_threshold` into
 * segments [seg_begin, seg_end) of the `ids` array.  The SAME launch sums every segment with its own lane group into
 * partials[s,:] (workspace, n_segments x dim floats) next to the light rows, then a second small kernel adds each heavy
 * row's partials in a fixed order (bitwise reproducible, no float atomics) and applies out_scale.
 *   heavy_rows [n_heavy] row ids; heavy_segptr [n_heavy+1] offsets into the segment arrays.  n_heavy == 0: no plan.
 */

/* ------------------------------------------------------------------------------------------------
 * DEVICE: query embedding bag, mode='mean' (K2).  Replaces nn.EmbeddingBag(mode='mean') forward/backward,
 * Models/EmbeddingLayers.py:79,100-104.  `words` are row ids into `table` (already +1 shifted, Dataset.py:168).
 *   fwd: out[q,:]  = ( sum_{k in bag q} table[words[k],:] ) / len(q)          (0 for an empty bag)
 *   bwd: dtable[w,:] = sum_{entries k with words[k]==w} dout[bag(k),:] * inv_len[bag(k)]
 *        given the transposed CSR (word_ptr [n_table_rows+1], word_bags [nnz]) from ihg_transpose_csr.
 */
int ihg_bag_mean_fwd(const float* table, int64_t ld_table, const int32_t* bag_ptr, const int32_t* words,
                     const float* bag_len, float* out, int64_t ld_out, int64_t n_bags, int32_t dim,
                     ihg_stream_t stream);
int ihg_bag_mean_bwd(const float* dout, int64_t ld_dout, const int32_t* word_ptr, const int32_t* word_bags,
                     const float* inv_len, float* dtable, int64_t ld_dtable, int64_t n_table_rows, int32_t dim,
                     ihg_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * DEVICE: interactive (order 2 / 3) node -> hyperedge step (K5 + K6 fused).
 * Replaces FeatureInteractor.forward orders 2 and 3 (Models/CommonLayers.py:70-85): the [E, k*d]
 * concatenation is never materialised.
 *
 *   fwd: out[e,:] = p[u,:] + p[q,:] + p[i,:]
 *                 + W_uq (h[u]*h[q]) + W_qi (h[q]*h[i]) + W_iu (h[i]*h[u]) [+ W_uqi (h[u]*h[q]*h[i])]
 *        (u,q,i) = i3[e,:];  w is the reference's aggregation.weight, row-major [dim, k*dim] with
 *        k = 6 (order 2) or 7 (order 3); only its product blocks (columns >= 3*dim) are read here.  The
 *        first-order blocks and the bias are hoisted to node level by the caller:
 *        p[v,:] = W_type(v) h[v,:] (+ bias on user rows), N*d*d flops instead of E*3*d*d.
 *   bwd: given dout [E, dim]:
 *        g[e,s,:]  (s = 0,1,2 for u,q,i; [E,3,dim] contiguous) = d loss / d h[member s of e] through the
 *                   product terms only; the caller finishes with ihg_node_segment_sum per node type.
 *        dw[:, 3*dim:]  = gradient of the product blocks of w (first-order columns are left untouched).
 *        `workspace` must hold ihg_interact_bwd_workspace_bytes(...) bytes (per-workgroup partial dW slabs,
 *        reduced in a fixed order - bitwise reproducible).
 *   Both directions take a caller-owned, 16-byte aligned device `workspace` of ihg_interact_{fwd,bwd}_workspace_bytes
 *   bytes: the product blocks of w re-packed into MFMA fragment order (+ the dW slabs for bwd).  For dim in
 *   {32, 64, 128, 256} with 16-byte aligned rows the contraction runs on the matrix cores in exact fp32
 *   (v_mfma_f32_32x32x2_f32 / 16x16x4_f32); every other shape takes a scalar kernel with the same results.
 *   Orders 2 and 3 at dim 64 / 128 / 256 (order 2 forward: 64 / 128) and the dim-128 / 256 node-level maps of ihg_node_linear_* multiply through three exact bf16
 *   terms per fp32 operand instead - six v_mfma_f32_16x16x32_bf16 products per multiply, fp32 accumulation, an error at or
 *   below the fp32-MFMA kernels' (csrc/split_arith.hip).  The environment variable IHG_INTERACT_ARITH=f32, read at every
 *   call, keeps those shapes on the fp32-MFMA kernels.
 * dw == NULL (here and in ihg_interact_bwd_user_reduced): member gradients only - the caller takes the product blocks' weight gradients from
 * ihg_node_interact_bwd_weight.
 */
/* The forward's workspace, in floats and in this order (B = 3 product blocks at order 2, 4 at order 3; 0 bytes unless dim is 32 / 64 / 128 / 256 and order 2 / 3;
 * n_edges does not enter):
 *   B dim^2              the product blocks of w in fp32 MFMA fragment order
 *   6 dim^2 (dim >= 64)  planes: the split kernel's weight image - three bf16 planes of four block slots at either order */
int64_t ihg_interact_fwd_workspace_bytes(int64_t n_edges, int32_t dim, int32_t order);

int ihg_interact_fwd(const float* h, int64_t ld_h, const float* p, int64_t ld_p, const int32_t* i3,
                     const float* w, int64_t ld_w, int32_t order,
                     float* out, int64_t ld_out, void* workspace, int64_t workspace_bytes,
                     int64_t n_edges, int32_t dim, ihg_stream_t stream);

/* The backward's workspace (all ihg_interact_bwd* entry points), in floats and in this order (B, the widths and n_edges as above):
 *   B dim^2              the product blocks of w in fp32 MFMA fragment order
 *   S B dim^2            weight-gradient slabs: S = 512 at dim 32 / 64, 256 at dim 128, 32 at dim 256
 *   2 R dim              boundary runs of the user-reduced forms, values: two per tile range, sized for R = 256 ranges (dim 32: 2,048)
 *   2 R dim              the same for the users' first-order gradient (ihg_interact_bwd_gathered_first_order)
 *   2 R                  their users (int32)
 *   6 dim^2 (dim >= 64)  planes: the member kernel's weight image (two fp16 planes of four block slots, the weight columns' scales and inverses: 4 dim^2 + 8 dim of it)
 *   1,024 B + 16 + 2,048 x 320 (dim 32)   the narrow member kernel's image: packed blocks, padding, a dump region per tile range */
int64_t ihg_interact_bwd_workspace_bytes(int64_t n_edges, int32_t dim, int32_t order);

int ihg_interact_bwd(const float* h, int64_t ld_h, const int32_t* i3,
                     const float* w, int64_t ld_w, int32_t order,
                     const float* dout, int64_t ld_dout,
                     float* g, float* dw, int64_t ld_dw,
                     void* workspace, int64_t workspace_bytes,
                     int64_t n_edges, int32_t dim, ihg_stream_t stream);

/* The same backward with the USER slot of the member gradients reduced on chip (hyperedges must be numbered so that i3[:,0] is
 * non-decreasing, i.e. sorted by user, as ihgnn_amd's layout numbers them): g2 is [n_edges, 2, dim] (query slot, item slot) and
 * rows [0, n_users) of dh receive, for every user with hyperedges, the sum of its user-slot gradients in hyperedge order - exactly
 * what ihg_node_segment_sum over the user's incidence list would have produced from the [n_edges, 3, dim] buffer.  Rows of users
 * without hyperedges are not written (pre-zero them).  A third less written here and a third less read by the K7 pass over g2.
 * Available where ihg_interact_bwd_user_reduced_supported says so (dim 32, 128; dim 64 and 256 with the split arithmetic on); workspace as
 * for ihg_interact_bwd.  A caller that produces g2 in hyperedge chunks cuts them where the user changes: every call writes the rows
 * of the users whose hyperedges it was given.
 */
int32_t ihg_interact_bwd_user_reduced_supported(int32_t dim, int32_t order, int64_t ld_h);
int ihg_interact_bwd_user_reduced(const float* h, int64_t ld_h, const int32_t* i3, const float* w, int64_t ld_w, int32_t order,
                                  const float* dout, int64_t ld_dout, float* g2, float* dh, int64_t ld_dh, float* dw, int64_t ld_dw,
                                  void* workspace, int64_t workspace_bytes, int64_t n_edges, int32_t dim, ihg_stream_t stream);

/* The user-reduced member gradients (no weight gradients: dw as NULL above) from cotangent rows that were written ALREADY SCALED AND TAKEN APART by
 * ihg_edge_gather_sum_planes: planes_rows is [n_edges][2][dim] fp16 (4 dim bytes per row, like the fp32 row it stands for), inv_scale [n_edges] the rows' inverse
 * powers of two.  The kernel's eight column parts (dim 256) then copy the row's pieces instead of each finding its maximum, scaling and splitting it again; results
 * are bit-identical to ihg_interact_bwd_user_reduced on the fp32 rows.  Reference: the same lines as ihg_interact_bwd (Models/CommonLayers.py:70-85, autograd's backward).
 */
int32_t ihg_interact_bwd_user_reduced_planes_supported(int32_t dim, int32_t order, int64_t ld_h);
int ihg_interact_bwd_user_reduced_planes(const float* h, int64_t ld_h, const int32_t* i3, const float* w, int64_t ld_w, int32_t order,
                                         const void* planes_rows, const float* inv_scale, float* g2, float* dh, int64_t ld_dh,
                                         void* workspace, int64_t workspace_bytes, int64_t n_edges, int32_t dim, ihg_stream_t stream);

/* The user-reduced backward fused with the transpose of the hyperedge -> node pass that follows the interactive step in an IHGNN layer
 * (Models/GnnLayers.py:229-236: Y = Dv^-1 H Ef): the caller has the NODE-level cotangent dy [n_nodes, dim], and the hyperedge
 * cotangent dout[e] = sum over the three members m of dy_scale[m] * dy[m] (dy_scale NULL: 1) - what ihg_edge_gather_sum would
 * have produced - is formed inside the member-gradient kernel from three gathered rows; it is left in `dout` [n_edges, dim]
 * (written, not read) for the weight gradients here and for the caller's first-order scatter.  Everything else as
 * ihg_interact_bwd_user_reduced.  Available where ihg_interact_bwd_gathered_supported says so (dim 32; dim 64 and 128 with the split arithmetic on).
 * dw == NULL: member gradients and dout only (the weight gradients come from ihg_node_interact_bwd_weight); then dout == NULL as well: the
 * hyperedges' cotangents are not stored at all (the caller takes the first-order gradient from dy by the two-hop operator).
 */
int32_t ihg_interact_bwd_gathered_supported(int32_t dim, int32_t order, int64_t ld_h, int64_t ld_dy);
int ihg_interact_bwd_gathered(const float* h, int64_t ld_h, const int32_t* i3, const float* w, int64_t ld_w, int32_t order,
                              const float* dy, int64_t ld_dy, const float* dy_scale, float* dout, int64_t ld_dout,
                              float* g2, float* dh, int64_t ld_dh, float* dw, int64_t ld_dw,
                              void* workspace, int64_t workspace_bytes, int64_t n_edges, int32_t dim, ihg_stream_t stream);

/* ihg_interact_bwd_gathered that also leaves the USERS' rows of the first-order gradient: hyperedges are numbered by user, so
 *   dp[u] = sum over the hyperedges e of user u of dout[e]
 * is a sum over u's contiguous run of the cotangents the kernel forms anyway; it is added up on chip in hyperedge order (runs that cross the kernel's tile
 * ranges: in range order) and written to dp [n_nodes, ld_dp] (ld_dp >= dim) for every user that has a hyperedge.  Rows of users without hyperedges and of
 * query / item nodes are NOT written: the caller zeroes the former (ihg_zero_rows) and takes the latter from ihg_node_segment_sum over the two-hop list
 * with `rows`.  Needs hyperedge lists without multiplicities (sum_run dout = deg(u) D[u] + the two-hop sum only then).  Everything else, bit for bit, as
 * ihg_interact_bwd_gathered.  Available where ihg_interact_bwd_gathered_first_order_supported says so (dim 128 with the split arithmetic on).
 */
int32_t ihg_interact_bwd_gathered_first_order_supported(int32_t dim, int32_t order, int64_t ld_h, int64_t ld_dy);
int ihg_interact_bwd_gathered_first_order(const float* h, int64_t ld_h, const int32_t* i3, const float* w, int64_t ld_w, int32_t order,
                                          const float* dy, int64_t ld_dy, const float* dy_scale, float* dout, int64_t ld_dout,
                                          float* g2, float* dh, int64_t ld_dh, float* dp, int64_t ld_dp, float* dw, int64_t ld_dw,
                                          void* workspace, int64_t workspace_bytes, int64_t n_edges, int32_t dim, ihg_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * The interactive layer in its NODE-LEVEL form: out = out_scale * H FeatureInteractor(h) without any [n_edges, dim] tensor.
 * Replaces, for the layer as a whole, the reference's FeatureInteractor.forward + torch.sparse.mm(norm_factor * H, .)
 * (CommonLayers.py:70-85, GnnLayers.py:229-236): for a fixed node every product term of a hyperedge feature has the node's own feature
 * as a constant factor, so the sum over the node's hyperedges is a linear map of deg(v) h[v], three sums over the OTHER two members
 * (a_e, b_e) of its hyperedges and their products with h[v].  Two calls:
 *
 * ihg_node_pair_sums: sums[v] = [ sum_e h[a_e] | sum_e h[b_e] | sum_e h[a_e] * h[b_e] ]  (3 dim floats per node; * elementwise).
 *   pair_ptr / pair_ids: CSR over the nodes with 2 ids per incident hyperedge - (query, item) for a user, (user, item) for a query,
 *   (user, query) for an item; the split-row plan is ihg_node_segment_sum's, with segments of even length.  Any dim % 4 == 0.
 *   pair_weight (optional, one float per PAIR, i.e. per two ids): the pair enters all three sums that many times - the multiplicity of its hyperedge in a
 *   layout that keeps each distinct (user, query, item) triple once (duplicates are distinct hyperedges in the reference, Helpers/Graph.py:107-118).
 *
 * ihg_node_interact_fwd: out[v] = out_scale[v] * ( degree[v] (A_t h[v] + bias) + the typed blocks of w applied to the sums and their
 *   products with h[v] ), w = [A_u | A_q | A_i | W_uq | W_qi | W_iu (| W_uqi)] as in ihg_interact_fwd, rows grouped by type_begin[4]
 *   (host array).  degree: the node's hyperedge count as float (0 for an isolated node); out_scale / bias may be NULL.  Available where
 *   ihg_node_interact_fwd_supported says so (dim 64 / 128 / 256, split arithmetic on: IHG_INTERACT_ARITH != f32); the hyperedge form (ihg_interact_fwd +
 *   ihg_node_segment_sum) is the path everywhere else and gives the same rows to the tolerance of DESIGN.md section 5.
 */
int ihg_node_pair_sums(const float* h, int64_t ld_h, const int32_t* pair_ptr, const int32_t* pair_ids, const int32_t* row_order, float* sums,
                       int64_t ld_sums, int64_t n_rows, int32_t dim, int32_t heavy_threshold, const int32_t* seg_begin, const int32_t* seg_end,
                       int64_t n_segments, const int32_t* heavy_rows, const int32_t* heavy_segptr, int64_t n_heavy, float* partials,
                       const float* pair_weight, ihg_stream_t stream);
int32_t ihg_node_interact_fwd_supported(int32_t dim, int32_t order, int64_t ld_h, int64_t ld_sums, int64_t ld_out);
/* The node-level forward's workspace is one weight image, in floats (0 bytes at any other dim):
 *   dim 32:              3 x 7 x 1,024: every node type's seven blocks in fp32 MFMA fragment order
 *   dim 64 / 128 / 256:  24 dim^2 (two fp16 planes of eight block slots per node type) | 3 dim (the weight rows' scales) | 3 dim (their inverses) */
int64_t ihg_node_interact_fwd_workspace_bytes(int32_t dim);
int ihg_node_interact_fwd(const float* h, int64_t ld_h, const float* sums, int64_t ld_sums, const float* degree, const float* out_scale, const float* bias,
                          const float* w, int64_t ld_w, int32_t order, const int64_t* type_begin, float* out, int64_t ld_out, void* workspace,
                          int64_t workspace_bytes, int32_t dim, ihg_stream_t stream);

/* ihg_node_interact_bwd_weight: dw[:, 3 dim ..] (the product blocks W_uq, W_qi, W_iu (, W_uqi)) of the layer above from node-level data only:
 *   d W_block = sum over the nodes of (dy_scale[v] dy[v]) x X_block[v]^T, X = h * sums_a | h * sums_b | sums_ab | h * sums_ab assigned to the blocks of w by
 *   node type - N rows instead of n_edges hyperedges, no gathers.  dy: the layer output's cotangent [N, dim]; dy_scale (NULL: 1): the out_scale of the
 *   forward.  The first-order blocks dw[:, :3 dim] are not written (ihg_node_linear_bwd_weight has them).  With this, ihg_interact_bwd_gathered is called
 *   with dw == NULL (member gradients only).  Available where ihg_node_interact_bwd_weight_supported says so (dim 64 / 128 / 256, split arithmetic on: IHG_INTERACT_ARITH != f32).
 */
int32_t ihg_node_interact_bwd_weight_supported(int32_t dim, int32_t order, int64_t ld_h, int64_t ld_sums, int64_t ld_dy);
/* Its workspace is one region, in floats: R slabs of dim x B dim (B = 3 at order 2, 4 at order 3), one per row range of the width's kernel -
 * R = 512 at dim 32, 256 at dim 64, 128 at dim 128, 32 at dim 256 (0 bytes at any other dim) */
int64_t ihg_node_interact_bwd_weight_workspace_bytes(int32_t dim, int32_t order);
int ihg_node_interact_bwd_weight(const float* h, int64_t ld_h, const float* sums, int64_t ld_sums, const float* dy, int64_t ld_dy, const float* dy_scale, int32_t order,
                                 const int64_t* type_begin, float* dw, int64_t ld_dw, void* workspace, int64_t workspace_bytes, int32_t dim, ihg_stream_t stream);


/* ------------------------------------------------------------------------------------------------
 * DEVICE: node-level dense transforms (K4 and the hoisted first-order blocks of K6).
 * Replaces nn.Linear(d, d) `feature_transform` (Models/GnnLayers.py:145, 224) and the u / q / i column blocks of
 * `aggregation` (Models/CommonLayers.py:43, 55, 64-66, 81-85) once they are applied per node instead of per hyperedge,
 * plus the autograd backward of both (torch issues a [d x N] x [N x d] rocBLAS GEMM there that has no split-K).
 *
 * Nodes are typed by contiguous row ranges: type t = rows [type_begin[t], type_begin[t+1]), t = 0,1,2 (host int64[4]).
 * W_t[c][j] = w[c * ld_w + t * w_type_stride + j]; w_type_stride == 0 means one weight for every row.
 *   fwd        out[v,:] = x[v,:] * W_t^T  (+ bias_t if bit t of bias_type_mask is set; bias_t = bias + t * bias_type_stride,
 *              stride 0 = one bias vector shared by the masked types)
 *   bwd_input  dx[v,:]  = dout[v,:] * W_t
 *   bwd_weight dW_t     = sum_{v in t} dout[v,:]^T x[v,:]      (one dW over all rows if dw_type_stride == 0)
 *              dbias[c] = sum over rows of the masked types of dout[v,c]     (dbias may be NULL); with dbias_type_stride != 0
 *              (typed weights only) every type gets its own sum at dbias + t * dbias_type_stride, 0 for unmasked types.
 *              With dx != NULL the call also produces bwd_input's result (w typed exactly like dw: block t at column
 *              t * dw_type_stride); at dim 64 / 128 both come from one pass over dout, otherwise it runs the bwd_input launch itself.
 *              dx_accumulate != 0: dx += instead of dx = (a second contribution to the same gradient: the member gradients of
 *              the interactive step land in dx first, Models/CommonLayers.py:70-85) - where ihg_node_linear_bwd_accumulates
 *              says so (dim 64; dim 128 on the split-arithmetic kernels)
 * Any dim > 0: 32, 64, 128, 256 with 16-byte aligned rows run on the matrix cores, every other shape on the any-width
 * kernels (row-slab partials + a fixed-order sum for the weight gradient).  `workspace`: ihg_node_linear_workspace_bytes(dim)
 * bytes, 16-byte aligned.
 */
int64_t ihg_node_linear_workspace_bytes(int32_t dim);
int32_t ihg_node_linear_bwd_accumulates(int32_t dim, int64_t ld_dout, int64_t ld_x, int64_t ld_dx);
int ihg_node_linear_fwd(const float* x, int64_t ld_x, const float* w, int64_t ld_w, int64_t w_type_stride,
                        const float* bias, int32_t bias_type_mask, int64_t bias_type_stride, const int64_t* type_begin,
                        float* out, int64_t ld_out, void* workspace, int64_t workspace_bytes,
                        int32_t dim, ihg_stream_t stream);
int ihg_node_linear_bwd_input(const float* dout, int64_t ld_dout, const float* w, int64_t ld_w, int64_t w_type_stride,
                              const int64_t* type_begin, float* dx, int64_t ld_dx,
                              void* workspace, int64_t workspace_bytes, int32_t dim, ihg_stream_t stream);
int ihg_node_linear_bwd_weight(const float* dout, int64_t ld_dout, const float* x, int64_t ld_x,
                               const int64_t* type_begin, float* dw, int64_t ld_dw, int64_t dw_type_stride,
                               float* dbias, int32_t bias_type_mask, int64_t dbias_type_stride,
                               const float* w, int64_t ld_w, float* dx, int64_t ld_dx, int32_t dx_accumulate,
                               void* workspace, int64_t workspace_bytes, int32_t dim, ihg_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * DEVICE: batch tail - HEM scoring head over the layer outputs.
 * Replaces torch.cat(gnn_outputs, 1) + the three row gathers of RawGnn.forward (Models/RawGnn.py:122-131) and
 * HemPredictionLayer.forward (Models/PredictionLayers.py:30-43, dot-product branch) for a training batch, and their
 * autograd backward up to (not including) the scatter of duplicate rows.
 *   layers   HOST array of n_layers (<= 8) device pointers, layer l = [N, dim] with row stride ld
 *   rows     device int64 [3*batch]: global node rows of the batch's users, then queries, then items
 *   items    device int64 [batch]: 0-based item ids (index into bias [I])
 *   fwd      scores[r] = sum_l <X_l[item_r], lambda*X_l[query_r] + (1-lambda)*X_l[user_r]> + bias[items[r]]
 *   bwd      rowgrad [3*batch, ld_rowgrad >= n_layers*dim]: gradient contribution of batch row r to its user / query / item
 *            row (blocks 0 / 1 / 2) for the upstream gradient grad_scale * dscores[batch].  If ld_rowgrad > n_layers*dim,
 *            column n_layers*dim carries d bias: dscores[r] on the item row, 0 on the other two.
 * ihg_bce_with_logits: nn.BCEWithLogitsLoss() (mean) and d loss / d scores in one launch (Main.py:191, TrainTestHelper.py:132).
 * ihg_batch_scatter_add: dense[rows[k], c] += rowgrad[k, c] for k < n_rows <= 32768 (ihg_batch_scatter_max_rows()), duplicates summed in batch order
 *            without atomics or a sort (one wave per batch row; the first occurrence of a destination adds all later ones).
 *            A NEGATIVE rows[k] takes no part: its row is neither added anywhere nor matched with another row (the same holds in
 *            ihg_batch_combine, where leader[k] = 0 and rowgrad[k] stays as it is, and in ihg_batch_rows_add / _put, which skip it).
 *            Column c lands at dense[(c / block_width) * block_stride + row * ld_dense + c % block_width] - with
 *            block_width = dim, block_stride = N * dim every layer's gradient is its own contiguous [N, dim] matrix; if `tail`
 *            is given, the last column goes to tail[row - tail_row_offset] instead (d bias).  Replaces the
 *            index_put_(accumulate=True) that autograd issues for the three row gathers (RawGnn.py:128-131).
 */
int ihg_hem_score_fwd(const float* const* layers, int32_t n_layers, int64_t ld, int32_t dim,
                      const int64_t* rows, const int64_t* items, const float* bias, float lambda_muq,
                      float* scores, int64_t batch, ihg_stream_t stream);
int ihg_hem_score_bwd(const float* const* layers, int32_t n_layers, int64_t ld, int32_t dim,
                      const int64_t* rows, const float* dscores, float grad_scale, float lambda_muq,
                      float* rowgrad, int64_t ld_rowgrad, int64_t batch, ihg_stream_t stream);
int ihg_bce_with_logits(const float* scores, const float* labels, int64_t n, float* loss, float* dscores, ihg_stream_t stream);
/* Ranking losses (not in the reference, whose only objective is the BCE above) over scores [positives * (1 + k)] laid out as the batches are: the positives first, then
 * the k negatives of positive p at positives + p * k ..; loss and dscores [positives * (1 + k)] = d loss / d scores in one launch, no atomics, every sum in a fixed order
 * (bitwise repeatable).  A negative that equals its positive is a group member like any other.
 *   IHG_LOSS_BPR      mean over the positives * k pairs of softplus(s_pj - s_p)
 *   IHG_LOSS_SOFTMAX  mean over the positives of -log softmax(s_p, s_p1 .. s_pk)[0]: the positive against its own k negatives
 * Any positives >= 1 and k >= 1 with positives * (1 + k) <= INT32_MAX. */
#define IHG_LOSS_BPR 1
#define IHG_LOSS_SOFTMAX 2
int ihg_ranking_loss(const float* scores, int64_t positives, int32_t k, int32_t kind, float* loss, float* dscores, ihg_stream_t stream);
/* Hard negatives (dynamic negative sampling; not in the reference): scores [positives * (1 + pool)] are the positives followed by the `pool` candidates of positive p at
 * positives + p * pool ..; the `keep` candidates of a group that come first by (score descending, pool position ascending) are its negatives.  Score order is the order of
 * the monotone uint32 key of the float's bits - sign bit set: ~bits, otherwise bits | 0x80000000 - a strict total order over every bit pattern: a positive-sign NaN sorts
 * above +inf, a negative-sign NaN below -inf, -0.0 below +0.0.  Exactly `keep` candidates are selected per group whatever the input, NaN included.
 * One launch writes
 *   selected [positives, keep] int32: selected[p][r] = the pool position 0 .. pool-1 of group p's r-th best;
 *   loss: the objective over every positive and its selected negatives - IHG_LOSS_BCE: ihg_bce_with_logits with labels 1 / 0, mean over positives * (1 + keep);
 *         IHG_LOSS_BPR / IHG_LOSS_SOFTMAX: ihg_ranking_loss with k = keep (means over positives * keep / over positives);
 *   dscores [positives * (1 + pool)] = d loss / d scores, EVERY entry: exactly +0.0 on a candidate that is not selected.
 * No atomics; every sum runs in an order that is a function of (positives, pool, keep) alone, so two launches on the same input agree bit for bit.
 * 1 <= keep <= pool <= 256, positives >= 1, positives * (1 + pool) <= INT32_MAX; IHG_ERR_INVALID has launched nothing. */
#define IHG_LOSS_BCE 0
int ihg_hard_negative_loss(const float* scores, int64_t positives, int32_t pool, int32_t keep, int32_t kind, float* loss, float* dscores, int32_t* selected,
                           ihg_stream_t stream);
int64_t ihg_batch_scatter_workspace_bytes(int64_t n_rows);      /* 0, or -1 if n_rows > ihg_batch_scatter_max_rows() (caller scatters in row chunks) */
int32_t ihg_batch_scatter_max_rows(void);                        /* 32768: rows of one ihg_batch_scatter_add / ihg_batch_combine launch (its id list lives in LDS: <= 16384 rows in 64 KiB,
                                                                    beyond that - the union of the ranks' batches under the cotangent exchange - a 128 KiB instance) */
int ihg_batch_scatter_add(const float* rowgrad, int64_t ld_rowgrad, int32_t width, const int64_t* rows, int64_t n_rows,
                          float* dense, int64_t ld_dense, int32_t block_width, int64_t block_stride,
                          float* tail, int64_t tail_row_offset, int64_t tail_rows, ihg_stream_t stream);
/* The same combination without a destination, for gradients that are added into several matrices at different times (one
 * per layer output, as the backward reaches it): ihg_batch_combine sums the rows of equal destination INTO the first of them,
 * in place, and sets leader[k] = 1 on those first occurrences (0 elsewhere); ihg_batch_rows_add then does
 * dense[rows[k], 0:width] += src[k, 0:width] over the leader rows (src = any column window of the combined rowgrad), or, with
 * `tail`, tail[rows[k] - tail_row_offset] += src[k, 0].  Leaders have distinct destinations: no atomics, fixed order.
 * disjoint_block_rows (0 = n_rows): consecutive blocks of that many batch rows are known not to share destinations - the user,
 * query and item thirds of a batch - so equal destinations are only looked for inside a block. */
int ihg_batch_combine(float* rowgrad, int64_t ld_rowgrad, int32_t width, const int64_t* rows, int64_t n_rows,
                      int64_t disjoint_block_rows, int32_t* leader, ihg_stream_t stream);
int ihg_batch_rows_add(const float* src, int64_t ld_src, int32_t width, const int64_t* rows, const int32_t* leader, int64_t n_rows,
                       float* dense, int64_t ld_dense, float* tail, int64_t tail_row_offset, int64_t tail_rows, ihg_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * DEVICE: the query transform, Gs.Query.transform == 'activation' (Helpers/GlobalSettings.py:68-76): the bag means m [n_rows, dim] of the queries go through
 * nn.Sequential(nn.Linear(dim, dim), Gs.Query.transform_activation()) (Models/EmbeddingLayers.py:40-44, applied at 83-84), act = nn.ReLU or nn.Tanh.
 *   ihg_rows_linear_act_fwd   out[r] = act(x[r] w^T + bias)  - the row GEMM of ihg_node_linear_fwd (one weight, no node types) with the activation in its epilogue;
 *                             `out` may be a column slice of a wider matrix (any ld_out >= dim, no alignment asked of it).  Replaces EmbeddingLayers.py:83-84.
 *   ihg_rows_linear_act_bwd   autograd's backward of the same two modules in one call: reads dy and y = out, forms dz = dy * act'(y) as dy is loaded
 *                             (act'(y) = [y > 0] for ReLU, 1 - y^2 for Tanh: neither the pre-activation nor dz is ever stored), and writes
 *                             dw[c][j] = sum_r dz[r][c] x[r][j], dbias[c] = sum_r dz[r][c] (NULL: skipped) - per-workgroup slabs added in a fixed order, no atomics,
 *                             bitwise reproducible - and dx = dz w (NULL: skipped).
 * dim 32 / 64 / 128 / 256 with 16-byte aligned x / dy / y rows run on the matrix cores: the forward at dim 128 / 256 in the arithmetic of ihg_node_linear_fwd (two fp16
 * terms per operand by default - when `out` is 16-byte aligned with ld_out % 4 == 0 -, fp32 MFMA under IHG_INTERACT_ARITH=f32); dim 32 / 64 and the backward at every
 * tiled width: fp32 MFMA (v_mfma_f32_32x32x2_f32) in either mode.  Every other shape: the any-width kernels.  n_rows == 0: the forward writes nothing, the backward
 * zeroes dw / dbias.  `workspace`: ihg_node_linear_workspace_bytes(dim) bytes, 16-byte aligned.
 */
#define IHG_ACT_RELU          1   /* nn.ReLU */
#define IHG_ACT_TANH          2   /* nn.Tanh */
int ihg_rows_linear_act_fwd(const float* x, int64_t ld_x, const float* w, int64_t ld_w, const float* bias, int32_t activation, float* out, int64_t ld_out,
                            int64_t n_rows, void* workspace, int64_t workspace_bytes, int32_t dim, ihg_stream_t stream);
int ihg_rows_linear_act_bwd(const float* dy, int64_t ld_dy, const float* y, int64_t ld_y, const float* x, int64_t ld_x, const float* w, int64_t ld_w,
                            int32_t activation, float* dw, int64_t ld_dw, float* dbias, float* dx, int64_t ld_dx, int64_t n_rows, void* workspace,
                            int64_t workspace_bytes, int32_t dim, ihg_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * DEVICE: composition of the two linear maps of a first-order layer - `feature_transform` (W [d,d], b; Models/GnnLayers.py:224)
 * followed by the first-order blocks of `aggregation` (A [d,3d] = A_u | A_q | A_i, bias c; Models/CommonLayers.py:60-66) with
 * nothing non-linear between them: node type t sees x (A_t W)^T + (A_t b + [t == user] c), which is what
 * ihg_node_linear_fwd then applies in one pass (typed weights, per-type bias).
 *   fwd   w_eff[i][t d + j] = sum_k A[i][t d + k] W[k][j]      b_eff[t][i] = sum_k A[i][t d + k] b[k] + (t == 0 ? c[i] : 0)
 *   bwd   gradients of both outputs back to A (da [d,3d]), c (dc, may be NULL), W (dw [d,d]) and b (db)
 * Tiny (3 d^3 multiply-adds), one thread per output element, sums in index order.
 */
int ihg_compose_first_order_fwd(const float* a, int64_t ld_a, const float* c, const float* w, int64_t ld_w, const float* b,
                                float* w_eff, int64_t ld_w_eff, float* b_eff, int32_t dim, ihg_stream_t stream);
int ihg_compose_first_order_bwd(const float* a, int64_t ld_a, const float* w, int64_t ld_w, const float* b,
                                const float* dw_eff, int64_t ld_dw_eff, const float* db_eff,
                                float* da, int64_t ld_da, float* dc, float* dw, int64_t ld_dw, float* db,
                                int32_t dim, ihg_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * DEVICE: the optimiser step of the training loop (Main.py:192 `torch.optim.Adam(model.parameters(), lr, weight_decay=...)`,
 * stepped in TrainTestHelper.py:139-143), for all parameters in one launch per 24 tensors.  Same update as torch.optim.Adam
 * (amsgrad off, maximize off): g += wd * p; m += (g - m)(1 - b1); v = b2 v + (1 - b2) g^2;
 * p -= lr / (1 - b1^t) * m / (sqrt(v) / sqrt(1 - b2^t) + eps), t = `step` >= 1 (the caller counts).  `tensors` is a HOST array.
 * Every entry is checked before the first launch (count >= 0; four non-null pointers where count > 0): a call that returns
 * IHG_ERR_INVALID has updated nothing.  Empty tensors (count == 0) are skipped.
 */
typedef struct ihg_adam_tensor {
    float* param;
    const float* grad;
    float* exp_avg;
    float* exp_avg_sq;
    int64_t count;
} ihg_adam_tensor;
int ihg_adam_step(const ihg_adam_tensor* tensors, int32_t n_tensors, float lr, float beta1, float beta2, float eps,
                  float weight_decay, int64_t step, ihg_stream_t stream);
/* The same update with the two step-dependent scalars read from DEVICE memory when the kernel runs: step_scalars[0] = lr / (1 - beta1^t),
 * step_scalars[1] = sqrt(1 - beta2^t).  For a launch recorded in a hipGraph (ihgnn_amd/captured_step.py): the host refreshes the two floats
 * before every replay, the recorded launch stays the same. */
int ihg_adam_step_device_scalars(const ihg_adam_tensor* tensors, int32_t n_tensors, float beta1, float beta2, float eps, float weight_decay,
                                 const float* step_scalars, ihg_stream_t stream);

/* Clipping by the global L2 norm of the gradients, torch.nn.utils.clip_grad_norm_(params, max_norm, norm_type=2, error_if_nonfinite=False) followed by Adam.step()
 * (nothing in the reference, whose step has no clipping), in three launches around the table Adam takes:
 *
 *   ihg_grad_sqnorm   *sum (a DEVICE double) = sum of grad^2 over every tensor of the table (it reads `grad` and `count` only).  One partial per 4,096 elements of a
 *                     tensor in `workspace` (ihg_grad_sqnorm_workspace_bytes(tensors, n_tensors) = 8 bytes per chunk, 8-byte aligned; -1 for a bad table), every
 *                     element squared and added in double in a fixed order, the partials added in a fixed order by one workgroup: no atomics, the same bits on
 *                     every call whatever the grid, and a float's square never overflows.  An empty table gives 0.
 *   ihg_clip_record   clip[0] = norm = (float) sqrt(*sum); clip[1] = coef = max_norm / (norm + 1e-6f), at most 1 (a NaN stays a NaN, as torch.clamp(max=1) leaves
 *                     it).  `stats` (may be null), three floats the caller zeroes once: the largest norm so far, the calls with coef < 1, the calls.  max_norm >= 0;
 *                     +inf is allowed (coef = 1 unless the norm is inf or NaN).  Separate from the sum so that ranks that hold shards of the gradient can add their
 *                     sums in between.
 *   ihg_adam_step_clipped / _clipped_device_scalars   ihg_adam_step / ihg_adam_step_device_scalars on g * clip[1] (the product is formed before the weight-decay
 *                     term, the order torch gives).  `grad` itself is NOT rewritten - the one difference from torch; the scaled gradient is grad * clip[1].
 *                     With clip[1] == 1 the result is bit for bit the unclipped entry's. */
int64_t ihg_grad_sqnorm_workspace_bytes(const ihg_adam_tensor* tensors, int32_t n_tensors);
int ihg_grad_sqnorm(const ihg_adam_tensor* tensors, int32_t n_tensors, void* workspace, int64_t workspace_bytes, double* sum, ihg_stream_t stream);
int ihg_clip_record(const double* sum, float max_norm, float* clip, float* stats, ihg_stream_t stream);
int ihg_adam_step_clipped(const ihg_adam_tensor* tensors, int32_t n_tensors, float lr, float beta1, float beta2, float eps,
                          float weight_decay, int64_t step, const float* clip, ihg_stream_t stream);
int ihg_adam_step_clipped_device_scalars(const ihg_adam_tensor* tensors, int32_t n_tensors, float beta1, float beta2, float eps, float weight_decay,
                                         const float* step_scalars, const float* clip, ihg_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * DEVICE: negative sampling of a training batch.  Replaces `random.sample(range(item_count), k)` per positive in
 * GraphDataset.__getitem__ (Dataset.py:107-109): out[row][0..k) = k DISTINCT item ids, uniform over [0, n_items), the positive
 * itself not excluded (as in the reference).  A pure function of (seed, counter, row): the caller advances `counter` per batch.
 * Not the reference's Mersenne-Twister stream - same distribution, different draws.  k <= 16.
 */
int ihg_sample_negatives(uint64_t seed, uint64_t counter, int64_t n_rows, int64_t n_items, int32_t k, int64_t* out, ihg_stream_t stream);
/* The same draw continued past 16, for a pool of candidates per positive: out [n_rows, m] int64, m DISTINCT values below n_items per row, 1 <= m <= min(256, n_items).
 * Row r's stream is ihg_sample_negatives' key(seed, counter, r); attempts are counted from 0, attempt a yields umulhi(mix64(key + a * 0x2545F4914F6CDD1D), n_items), an
 * attempt is accepted iff its value differs from every value accepted before it, and the first m accepted values, in attempt order, are the row.  So the first c columns
 * of a call with m are what a call with c gives, and for c <= 16 they are ihg_sample_negatives' bits.  IHG_ERR_INVALID (m out of range, a null `out` with rows to write)
 * has launched nothing; n_rows == 0 returns IHG_OK. */
int ihg_sample_pool(uint64_t seed, uint64_t counter, int64_t n_rows, int64_t n_items, int32_t m, int64_t* out, ihg_stream_t stream);
/* The pool draw with a per-row list of values that are never drawn (negatives outside what the row's user has bought): out [n_rows, m] int64.  Lists are a CSR in the
 * layout of per-search exclusion lists: list l = list_items[list_ptr[l] .. list_ptr[l + 1]) (list_ptr int64 [n_lists + 1], list_items int32), every list ascending and
 * distinct, values in [0, n_items).  Row r has list l = list_of_row[r] (int64 [n_rows]); an l outside [0, n_lists) means an empty list, and list_ptr is not read for it.
 * Sequential definition: row r walks ihg_sample_negatives' stream - key(seed, counter, r), attempts counted from 0, attempt a yields
 * umulhi(mix64(key + a * 0x2545F4914F6CDD1D), n_items); a value is accepted iff it is not in the row's list and differs from every value accepted before it; out[r][0..m)
 * are the first m accepted values, in attempt order.  So row r is row r of the unfiltered stream with the listed values deleted; with all lists empty the output is
 * ihg_sample_pool's bit for bit (for m <= 16: ihg_sample_negatives'); the first c columns of a call with m are what a call with c gives.  One kernel serves every m.
 * max_list_len is the caller's promise that no list is longer, computed on the host from its copy of list_ptr and never read back from the device: the draw ends
 * because m + max_list_len <= n_items leaves every row m values to find.  IHG_ERR_INVALID unless 1 <= m <= min(256, n_items), n_lists >= 1, max_list_len >= 0 and
 * m + max_list_len <= n_items, and on a null pointer with rows to write: it has launched and written nothing.  n_rows == 0 returns IHG_OK and launches nothing. */
int ihg_sample_pool_excluding(uint64_t seed, uint64_t counter, int64_t n_rows, int64_t n_items, int32_t m, const int64_t* list_of_row, int64_t n_lists,
                              const int64_t* list_ptr, const int32_t* list_items, int64_t max_list_len, int64_t* out, ihg_stream_t stream);
/* The pool draw with item weights (popularity-weighted negatives), with or without the per-row lists of ihg_sample_pool_excluding: out [n_rows, m] int64.  cum is int64
 * [n_items + 1], the running sum of integer item weights: cum[0] = 0, strictly ascending (every weight >= 1), cum[n_items] = total < 2^63.  The lists are the CSR of
 * ihg_sample_pool_excluding with its list_of_row and its rule that an l outside [0, n_lists) means an empty list; with n_lists == 0 the three list pointers may be null
 * and no row has a list.  Sequential definition: row r walks ihg_sample_negatives' stream - key(seed, counter, r), attempts counted from 0, attempt a yields the
 * threshold t = umulhi(mix64(key + a * 0x2545F4914F6CDD1D), total), and its value is the one i with cum[i] <= t < cum[i + 1]; a value is accepted iff it is not in the
 * row's list and differs from every value accepted before it; out[r][0..m) are the first m accepted values, in attempt order.  So item i is drawn with probability
 * (cum[i + 1] - cum[i]) / total per attempt, and the first accepted value follows the weights renormalised over the complement of the row's list.  With cum[i] = i the
 * output is ihg_sample_pool_excluding's bit for bit (no lists: ihg_sample_pool's; m <= 16: ihg_sample_negatives'), and so it is with every weight 2^32, because
 * umulhi(r, I * 2^32) >> 32 == umulhi(r, I); the first c columns of a call with m are what a call with c gives.  One kernel serves every m.  total and max_list_len
 * are the caller's promises, computed on the host and never read back from the device, and so is the strict ascent of cum, which this call cannot see: a table with a
 * zero weight, or a longer list, may keep a row from ever finding its m values.  IHG_ERR_INVALID unless 1 <= m <= min(256, n_items), n_items <= total < 2^63,
 * n_lists >= 0, max_list_len >= 0 and m + max_list_len <= n_items, and on a null pointer with rows to write (the list pointers only when n_lists > 0): it has launched
 * and written nothing.  n_rows == 0 returns IHG_OK and launches nothing. */
int ihg_sample_pool_weighted(uint64_t seed, uint64_t counter, int64_t n_rows, int64_t n_items, int32_t m, const int64_t* cum, int64_t total,
                             const int64_t* list_of_row, int64_t n_lists, const int64_t* list_ptr, const int32_t* list_items, int64_t max_list_len,
                             int64_t* out, ihg_stream_t stream);

/* DEVICE: one whole training batch in one launch, logged negatives included.  Replaces, for the n positives `edge_ids` of pos_triples [E, 3]
 * (user, query, item), GraphDataset.__getitem__ + collate_fn (Dataset.py:107-119, 282-291).  pack is the [4, n (1 + k)] array collate_fn builds, k = k_rand + k_logged,
 * rows users / queries / items / flags: columns [0, n) are the positives in edge_ids order with flag 1; column n + row k + slot is negative `slot` of positive `row`,
 * with the positive's user and query and flag 0.
 * The logged negatives (items the same (user, query) pair was shown and did not click) are lists in file order with repeats kept: pair_of_edge [E] = the pair of
 * every positive, list of pair p = neg_items[neg_ptr[p] .. neg_ptr[p + 1]).  With L the row's list and len its length, the reference's rule:
 *   len >= k_logged: k_logged entries of L at DISTINCT positions drawn uniformly (an item repeats where L repeats it), then k_rand random items;
 *   len <  k_logged: k - len random items, then all of L in file order.
 * Random items are distinct within the row, uniform over [0, n_items), the positive not excluded: ihg_sample_negatives' contract.
 * Two counter-based streams per row, both "c distinct values below m" by the same multiply-high draw with reject-and-redraw, attempts counted from 0:
 *   items:     key(seed, counter, row) of ihg_sample_negatives, m = n_items: the c random items of row r are bit for bit the first c entries of row r of
 *              ihg_sample_negatives(seed, counter, n, n_items, k), so k_logged = 0 reproduces that launch;
 *   positions: key(seed, counter, row) ^ 0xA0761D6478BD642F, m = len.
 * A pure function of (seed, counter, row).  k_rand >= 0, k_logged >= 0, 1 <= k <= min(16, n_items); the three list pointers may be null only when k_logged == 0;
 * ids in edge_ids must be in [0, E).  IHG_ERR_INVALID has launched nothing; n == 0 returns IHG_OK.
 */
int ihg_device_batch(uint64_t seed, uint64_t counter, const int64_t* pos_triples, const int64_t* edge_ids, int64_t n, const int32_t* pair_of_edge,
                     const int64_t* neg_ptr, const int32_t* neg_items, int64_t n_items, int32_t k_rand, int32_t k_logged, int64_t* pack, ihg_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * DEVICE: evaluation scoring with a running top-k.  Replaces, for `n_pairs` search logs at once, the per-log
 * sequence RawGnn.forward(u * ones(I), q * ones(I), None) (Models/RawGnn.py:124-137) -> HemPredictionLayer.forward
 * (Models/PredictionLayers.py:35-43) -> torch.sort(scores, descending=True)[:10] (Helpers/Metrics.py:60-61):
 *   score[c][i] = sum_k features[item_row0 + i][k] * (lambda * features[query_row0 + queries[c]][k] + (1 - lambda) * features[users[c]][k])
 *                 + item_bias[i]
 *   top_items[c][0..k) = the k items of highest score, best first; equal scores in ascending item order (a stable descending
 *   sort; the reference's sort is unstable on ties); top_scores[c][0..k) their scores.  With fewer than k items the tail is -1.
 * `features` is the cached [N, dim] propagation output (any row stride >= dim, dim <= ihg_score_topk_max_dim() = 1264: the mixed rows of 32 pairs
 * stay in LDS); k <= 10.
 * The [n_pairs, n_items] score matrix is never stored: 32 x 32 matrix-core tiles are reduced to per-lane top-k lists in registers.  Arithmetic: every row is
 * multiplied by a power of two and taken apart into two fp16 terms (hi + lo, 22 significand bits); a product is three v_mfma_f32_32x32x16_f16 partial products
 * accumulated in fp32 (relative error <= 3 x 2^-22 per product, as accurate as the fp32 matrix instructions on these sums - tests/test_gpu_parity.py); the item rows are
 * split once per call into the workspace.
 * Workspace: ihg_score_topk_workspace_bytes(n_pairs, n_items, dim) bytes; regions in order: the split item rows (MFMA fragments) | aux, 8 bytes per item | the partial
 * lists' scores | their item ids.  A workspace that is NULL, not 16-byte aligned or smaller answers IHG_ERR_WORKSPACE (so do ihg_score_topk_cosine and _deep).
 */
int32_t ihg_score_topk_max_dim(void);
int64_t ihg_score_topk_workspace_bytes(int64_t n_pairs, int64_t n_items, int32_t dim);
int ihg_score_topk(const float* features, int64_t ld, int32_t dim, int64_t query_row0, int64_t item_row0, int64_t n_items,
                   const float* item_bias, const int64_t* users, const int64_t* queries, float lambda_muq, int64_t n_pairs,
                   int32_t k, float* top_scores, int32_t* top_items, void* workspace, int64_t workspace_bytes, ihg_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * DEVICE: the input features X0 WITHOUT assembling them.  The reference concatenates rows 1.. of the user table, the queries' bag means and
 * rows 1.. of the item table into one [N, d] matrix every step (Models/RawGnn.py:112-113, Models/EmbeddingLayers.py:70-79) and autograd cuts the
 * gradient apart again: four [N, d]-sized copies per training step.  The *_typed entry points take, instead of one matrix, the address of the FIRST ROW
 * of every node type (a HOST array of 3 device pointers: users, queries, items; common row stride) - the layer-0 transform, its weight / input gradient,
 * the scoring head's layer-0 rows and the scatter of the batch rows' gradients read and write the tables in place.
 *   ihg_node_linear_fwd_typed          ihg_node_linear_fwd with x given as typed rows
 *   ihg_node_linear_bwd_weight_typed   ihg_node_linear_bwd_weight with x (and the optional input gradient dx) as typed rows; bit t of
 *                                      zero_row_before_mask: the row in front of dx_rows[t] (the padding row 0 of an embedding table's gradient) is zeroed
 *   ihg_hem_score_fwd_typed0 / ihg_hem_score_bwd_typed0   ihg_hem_score_fwd / _bwd with layer 0 given as typed rows (row stride ld0; layer0_rows NULL: every layer a
 *                                      plain matrix); _bwd multiplies the upstream gradient by *grad_scale_device (a DEVICE scalar, NULL: 1) as well - d loss of a
 *                                      backward pass, without a host read or a separate multiply launch.  rows_upper (optional, [3 batch]): the rows of the layers ABOVE
 *                                      layer 0 where those are numbered differently from layer 0's - a layout that leaves the isolated nodes (no hyperedge: every layer
 *                                      output is zero, Graph.py:120 / App. B 2) out of its own numbering while layer 0 is read from the embedding tables by the reference's
 *                                      node id; a negative entry = isolated: its rows above layer 0 count as zero (ihg_batch_rows_add / _put skip negative rows)
 *   ihg_batch_rows_put                 ihg_batch_rows_add into typed rows; assign != 0: dense[rows[k]] = src[k] on the leader rows (a gradient that is
 *                                      zero elsewhere and read at these rows only: no fill of the matrix)
 * Available where ihg_node_linear_typed_supported says so (dim 128 / 256 on the split-arithmetic kernels, row strides % 4 == 0, 16-byte aligned rows).
 */
int32_t ihg_node_linear_typed_supported(int32_t dim, int64_t ld_x, int64_t ld_out);
int ihg_node_linear_fwd_typed(const float* const* x_rows, int64_t ld_x, const float* w, int64_t ld_w, int64_t w_type_stride,
                              const float* bias, int32_t bias_type_mask, int64_t bias_type_stride, const int64_t* type_begin,
                              float* out, int64_t ld_out, void* workspace, int64_t workspace_bytes, int32_t dim, ihg_stream_t stream);
int ihg_node_linear_bwd_weight_typed(const float* dout, int64_t ld_dout, const float* const* x_rows, int64_t ld_x, const int64_t* type_begin,
                                     float* dw, int64_t ld_dw, int64_t dw_type_stride, float* dbias, int32_t bias_type_mask, int64_t dbias_type_stride,
                                     const float* w, int64_t ld_w, float* const* dx_rows, int64_t ld_dx, int32_t zero_row_before_mask,
                                     void* workspace, int64_t workspace_bytes, int32_t dim, ihg_stream_t stream);
int ihg_hem_score_fwd_typed0(const float* const* layers, int32_t n_layers, int64_t ld, int32_t dim, const float* const* layer0_rows, int64_t ld0,
                             const int64_t* type_begin, const int64_t* rows, const int64_t* rows_upper, const int64_t* items, const float* bias, float lambda_muq,
                             float* scores, int64_t batch, ihg_stream_t stream);
int ihg_hem_score_bwd_typed0(const float* const* layers, int32_t n_layers, int64_t ld, int32_t dim, const float* const* layer0_rows, int64_t ld0,
                             const int64_t* type_begin, const int64_t* rows, const int64_t* rows_upper, const float* dscores, const float* grad_scale_device,
                             float grad_scale, float lambda_muq, float* rowgrad, int64_t ld_rowgrad, int64_t batch, ihg_stream_t stream);
int ihg_batch_rows_put(const float* src, int64_t ld_src, int32_t width, const int64_t* rows, const int32_t* leader, int64_t n_rows,
                       float* const* dense_rows, int64_t ld_dense, const int64_t* type_begin, int32_t assign, ihg_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * DEVICE: the cosine-similarity head (Gs.Prediction.use_cosine_similarity, Models/PredictionLayers.py:38-40).  With a the item's concatenated row
 * [X_0 | .. | X_L][item] and m = lambda a[query] + (1 - lambda) a[user]:
 *   score = (a . m) / (max(||a||, 1e-8) max(||m||, 1e-8)) + bias[item]        (torch.cosine_similarity and its autograd: the norm's value is clamped, its derivative a / ||a|| is not)
 * The norms run over the whole concatenated row; an isolated node's zero rows above layer 0 (negative rows_upper) add zeros to the sums.
 *   ihg_hem_cosine_fwd   arguments of ihg_hem_score_fwd_typed0 (layer0_rows / ld0 / type_begin and rows_upper may be NULL) plus
 *                        stats [batch][4] floats, 16-byte aligned, caller-owned: stats[r] = {a . m, ||a||^2, ||m||^2, 0} of batch row r, kept for the backward
 *   ihg_hem_cosine_bwd   arguments of ihg_hem_score_bwd_typed0 plus the stats of the forward; writes the same [3 batch, ld_rowgrad] row gradients
 *                        (user rows | query rows | item rows, layer l in columns l dim .., d bias in column n_layers dim of the item rows where ld_rowgrad leaves room),
 *                        so everything downstream of them (ihg_batch_combine, ihg_batch_rows_add / _put, the cotangent exchange) is shared with the dot-product head
 *   ihg_score_topk_cosine  ihg_score_topk (same arguments, workspace and width limit) for this head: the item rows' and the mixed rows' inverse norms are folded into
 *                        the two scale factors the kernel multiplies its accumulators by; the loop over the items is the same code
 * No host reads, no allocations: a stream capture holds all three.
 */
int ihg_hem_cosine_fwd(const float* const* layers, int32_t n_layers, int64_t ld, int32_t dim, const float* const* layer0_rows, int64_t ld0,
                       const int64_t* type_begin, const int64_t* rows, const int64_t* rows_upper, const int64_t* items, const float* bias, float lambda_muq,
                       float* scores, float* stats, int64_t batch, ihg_stream_t stream);
int ihg_hem_cosine_bwd(const float* const* layers, int32_t n_layers, int64_t ld, int32_t dim, const float* const* layer0_rows, int64_t ld0,
                       const int64_t* type_begin, const int64_t* rows, const int64_t* rows_upper, const float* dscores, const float* stats,
                       const float* grad_scale_device, float grad_scale, float lambda_muq, float* rowgrad, int64_t ld_rowgrad, int64_t batch, ihg_stream_t stream);
int ihg_score_topk_cosine(const float* features, int64_t ld, int32_t dim, int64_t query_row0, int64_t item_row0, int64_t n_items,
                          const float* item_bias, const int64_t* users, const int64_t* queries, float lambda_muq, int64_t n_pairs,
                          int32_t k, float* top_scores, int32_t* top_items, void* workspace, int64_t workspace_bytes, ihg_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * DEVICE: ranking deeper than ten.  ihg_score_topk_deep is ihg_score_topk (its arguments, outputs, tie order, width limit and -1 tail; `cosine` != 0: the scores of
 * ihg_score_topk_cosine) for 1 <= k <= ihg_score_topk_max_k() = 128; any other k answers IHG_ERR_INVALID before anything is launched.
 * Scheme: the kernels keep their lists of ten per lane and the call runs in passes.  Per pair the workspace carries `count`, the ranks already in the output, and the
 * boundary, the last of them.  A pass scores every item again (the split item rows are prepared once per call) and lets a candidate into a lane's list only if it
 * ranks strictly after its pair's boundary; a workgroup whose pairs are all complete (count == min(k, n_items)) returns at once.  The pair's lists are sorted and
 * cover disjoint items, so with t = the best-ranking tenth entry over the FULL lists every item that ranks at or before t is in some list: a merge kernel (one wave per
 * pair, one head per list in registers) appends exactly those to the output, in order, stops at k and moves the boundary.  Every pass adds at least ten ranks to an
 * incomplete pair, so ceil(min(k, n_items) / 10) passes always suffice - 13 at k = 128 - and the call launches that fixed number of (score, merge) pairs: no
 * device-to-host read, no allocation, no atomics, no spinning; a stream capture holds it.  Random scores need one scoring pass at a catalogue's size; scores sorted by
 * item id, or all equal, need 8 at k = 128.  Every pass computes bit-identical scores (one kernel, one item order), so the boundary comparison is exact under ties and
 * two calls return the same bits; k <= 10 returns the bits of ihg_score_topk / ihg_score_topk_cosine.
 *   passes (optional, [n_pairs] int32): passes[c] = the number of passes that found pair c incomplete.
 * Workspace: ihg_score_topk_deep_workspace_bytes(n_pairs, n_items, dim, k) bytes: the regions of ihg_score_topk | the pairs' state (count, boundary, passes), 16 bytes per pair.
 */
int32_t ihg_score_topk_max_k(void);
int64_t ihg_score_topk_deep_workspace_bytes(int64_t n_pairs, int64_t n_items, int32_t dim, int32_t k);
int ihg_score_topk_deep(const float* features, int64_t ld, int32_t dim, int64_t query_row0, int64_t item_row0, int64_t n_items,
                        const float* item_bias, const int64_t* users, const int64_t* queries, float lambda_muq, int64_t n_pairs,
                        int32_t k, float* top_scores, int32_t* top_items, void* workspace, int64_t workspace_bytes, int32_t cosine, int32_t* passes,
                        ihg_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * DEVICE: answering a search.  ihg_search_topk is ihg_score_topk_deep - its outputs, tie order, -1 tail, 1 <= k <= 128, width limit, `cosine` and `passes`; no host
 * read, no allocation, no atomics, a stream capture holds it - with three additions, each what the model itself computes:
 *   query source   exactly one of `queries` ([n_pairs] node indices, as in ihg_score_topk) and `query_rows` is non-null.  query_rows is a [n_pairs, q_dim] float32
 *                  matrix (row stride ld_q >= q_dim, 1 <= q_dim <= dim): the query row of pair c is query_rows[c] in columns 0 .. q_dim and ZERO in columns
 *                  q_dim .. dim, which are never read from memory - a query that is not in the training graph is an isolated node: its layer-0 row is its words'
 *                  bag mean (or the query transform of it) and every layer output above is exactly zero (Helpers/Graph.py:120)
 *   no user        users[c] < 0: the mixed row of pair c is its query row itself, not lambda times it (the head's `user_feature is None` branch,
 *                  Models/PredictionLayers.py:34-37); under the cosine head its norm is the query row's
 *   candidates     item_mask: NULL (every item) or ceil(n_items / 32) uint32 words on the device, shared by all pairs; bit i % 32 of word i / 32 says that item i is
 *                  a candidate, bits at or past n_items are ignored.  An item that is no candidate never appears in the output; a pair is complete at
 *                  min(k, candidates), a count formed on the device inside the call, so complete pairs still let their workgroups return at once and
 *                  passes[c] <= ceil(min(k, candidates) / 10) (0 with no candidate: every output row is then the -1 tail).  The mask is applied where the item
 *                  rows are prepared, once per call: the scoring loop is that of ihg_score_topk_deep, and an all-ones mask returns the bits of a NULL mask.
 * With `queries`, no negative user and no mask the call returns the bits of ihg_score_topk_deep; with query_rows, those of ihg_score_topk_deep on a feature matrix
 * that has the rows appended (zero above q_dim) as further query rows.
 * IHG_ERR_INVALID before anything is launched: both or neither of queries / query_rows, q_dim outside 1 .. dim, ld_q < q_dim, k outside 1 .. 128, a workspace
 * smaller than ihg_search_topk_workspace_bytes(n_pairs, n_items, dim, k) (the regions of ihg_score_topk_deep | the 16-byte cell of the candidates' count) or not 16-byte aligned.  n_pairs == 0 with otherwise good sizes, query source (and lists)
 * returns IHG_OK before any pointer is looked at; so it does for every ranking entry point.
 */
int64_t ihg_search_topk_workspace_bytes(int64_t n_pairs, int64_t n_items, int32_t dim, int32_t k);
int ihg_search_topk(const float* features, int64_t ld, int32_t dim, int64_t query_row0, int64_t item_row0, int64_t n_items,
                    const float* item_bias, const int64_t* users, const int64_t* queries, const float* query_rows, int64_t ld_q, int32_t q_dim,
                    const uint32_t* item_mask, float lambda_muq, int64_t n_pairs, int32_t k, float* top_scores, int32_t* top_items,
                    void* workspace, int64_t workspace_bytes, int32_t cosine, int32_t* passes, ihg_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * DEVICE: a search that leaves out a different item set per pair ("not what this user already bought").  ihg_search_topk_excluding is ihg_search_topk - every
 * argument, output, tie order, -1 tail and limit - plus per-pair exclusion lists in CSR form:
 *   excl_ptr     int64 [n_excl_rows + 1], non-decreasing, excl_ptr[0] = 0
 *   excl_items   int32 [excl_ptr[n_excl_rows]]: run r is excl_items[excl_ptr[r] .. excl_ptr[r + 1]), STRICTLY ASCENDING, ids in [0, n_items)
 *   excl_row     int64 [n_pairs] or NULL: pair c leaves out run excl_row[c]; a negative entry leaves out nothing.  NULL: pair c leaves out run c, and
 *                n_excl_rows == n_pairs.  With excl_row one CSR of "items per user" serves any batch of searches without a copy per search.
 * An item of its pair's run is never ranked for that pair.  Pair c is complete at target_c = min(k, |candidates minus its run|) - an excluded id that item_mask
 * already removes is not subtracted twice - and the rest of its row is the (-FLT_MAX, -1) tail; passes[c] <= ceil(target_c / 10).  target_c is formed on the
 * device (two small launches per call, none per pass, no host read); the call still launches ceil(min(k, n_items) / 10) passes: an excluded item is in no lane's
 * list, so the lists stay exact over what remains and an incomplete pair still gains ten ranks per pass, or all that is left.
 * The scores of the items that remain are the bits of ihg_search_topk: the scoring loop computes every score with the same expression in the same item order, and
 * exclusion only decides whether a score may enter a lane's list - each lane follows the run of its pair with a cursor as its item ids ascend, so the cost grows
 * with the lists, not with pairs x items, and the memory is that of the lists plus 4 bytes per pair.  A pair whose run is empty gets the row ihg_search_topk
 * returns for it; with excl_ptr == NULL (then excl_items and excl_row are NULL too) the call launches what ihg_search_topk launches.
 * CONTRACT: the order inside a run, the range of the ids and of excl_row's entries (< n_excl_rows) live on the device and are the caller's to keep
 * (ops.exclusion_lists builds such lists); a run that is not strictly ascending gives a wrong ranking, not a fault.
 * IHG_ERR_INVALID before anything is launched, in ihg_search_topk's order: its size checks, its query-source checks, then excl_ptr without excl_items or the
 * reverse, excl_row without lists, n_excl_rows < 1 with lists (or != n_pairs with lists and no excl_row), then its null-pointer, width and list checks, then a
 * workspace smaller than ihg_search_topk_excluding_workspace_bytes(n_pairs, n_items, dim, k) (the regions of ihg_search_topk | target_c, 4 bytes per pair, rounded up to 16).
 */
int64_t ihg_search_topk_excluding_workspace_bytes(int64_t n_pairs, int64_t n_items, int32_t dim, int32_t k);
int ihg_search_topk_excluding(const float* features, int64_t ld, int32_t dim, int64_t query_row0, int64_t item_row0, int64_t n_items,
                              const float* item_bias, const int64_t* users, const int64_t* queries, const float* query_rows, int64_t ld_q, int32_t q_dim,
                              const uint32_t* item_mask, const int64_t* excl_ptr, const int32_t* excl_items, const int64_t* excl_row, int64_t n_excl_rows,
                              float lambda_muq, int64_t n_pairs, int32_t k, float* top_scores, int32_t* top_items, void* workspace, int64_t workspace_bytes,
                              int32_t cosine, int32_t* passes, ihg_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * DEVICE: re-ranking a shortlist per search (csrc/candidates.hip).  ihg_search_candidates takes what ihg_search_topk_excluding takes - the query source, users < 0,
 * the item mask, the exclusion lists, lambda, 1 <= k <= 128, `cosine`, `passes`, the outputs' tie order (higher score first, equal scores by ascending item id) and
 * their (-FLT_MAX, -1) tail - plus a CANDIDATE list per search in CSR form, and scores only the listed items: the work is sum_c |run_c| * dim, with no pass over the
 * n_items item rows, no prepare pass and no memory proportional to n_items.
 *   cand_ptr     int64 [n_cand_rows + 1], non-decreasing, cand_ptr[0] = 0, cand_ptr[n_cand_rows] = total
 *   cand_items   int32 [total]: run r is cand_items[cand_ptr[r] .. cand_ptr[r + 1]), STRICTLY ASCENDING, ids in [0, n_items)
 *   cand_row     int64 [n_pairs] or NULL: search c ranks run cand_row[c]; a negative or out-of-range entry is an empty run.  NULL: search c ranks run c, and
 *                n_cand_rows == n_pairs
 * An item is ranked for search c iff it is in run c, in item_mask (NULL: every item) and not in c's exclusion run.  Search c is complete at
 * target_c = min(k, the items so admitted); the rest of its row is the tail; passes[c] = ceil(target_c / 10), the trips of its selecting wave (0 with nothing admitted).
 *   all_scores   float32 [total] or NULL: the score of every list entry at its CSR slot, -inf (exactly) for an entry that the mask or the exclusion run removes, or
 *                whose id is outside [0, n_items); the top-k is the stable ranking of these very floats.  With cand_row a run's slots are written for the
 *                LOWEST-NUMBERED search that names it (a run that none names holds -inf): searches that share a run and differ in user or query need
 *                all_scores == NULL, which the caller sees to (the rows live on the device).
 * ARITHMETIC: plain fp32, NOT the bits of ihg_search_topk (two fp16 terms per operand on the matrix cores).  m = fma(lam, q, (1 - lam) u) (q alone for
 * users[c] < 0, zero past q_dim for an external row) is formed once per (search, chunk of 256 ids); G = min(16, the power of two at or above ceil(dim / 4)) lanes
 * own a candidate, lane g takes the four-column segments g, g + G, ... of the item row in one fma chain, a shuffle tree over G adds the partial sums, and
 * score = dot + bias[item]; cosine: dot / (max(sqrt(sum a^2), 1e-8) * max(sqrt(sum m^2), 1e-8)) + bias[item], both sums in that same order.  A score of -inf or NaN
 * is never ranked.  The result depends on no workspace byte and no launch order: two calls return equal bits.
 * Launches: the runs' plan (a wave per search; with cand_row it compares each entry with those below it), the scan of the scoring units, the scoring pass (a wave per
 * chunk of 256 ids of a run: a long run is spread over many waves) and the selecting pass (a wave per search).  A search that is not the first to name its run scores
 * it in its selecting wave instead (a slot holds one search's score), so the memory stays that of the lists.
 * ihg_search_candidates_max_dim() = 2048 is the widest row the mixed row's LDS image takes (the 1264 of the pair block of ihg_score_topk does not bind here).
 * CONTRACT: the order inside a run and the offsets live on the device and are the caller's to keep (ops.candidate_lists builds such lists); a run that is not
 * strictly ascending gives a wrong ranking, offsets outside [0, total] an empty run, an id outside [0, n_items) an entry that is never ranked - none of them a fault.
 * IHG_ERR_INVALID before anything is launched: ihg_search_topk_excluding's size, query-source and exclusion-list checks, then total < 0, n_cand_rows < 1 (or
 * != n_pairs without cand_row), then (n_pairs == 0 returns IHG_OK) a null pointer, dim > ihg_search_candidates_max_dim(), a workspace that is not 16-byte aligned or
 * smaller than ihg_search_candidates_workspace_bytes(n_pairs, total, dim, k) ; regions in order: the entries' scores, 4 total (rounded up to 16) | the scoring units' scan,
 * 8 (n_pairs + 1) (rounded up to 16) | the searches' runs, 16 n_pairs.
 */
int32_t ihg_search_candidates_max_dim(void);
int64_t ihg_search_candidates_workspace_bytes(int64_t n_pairs, int64_t total, int32_t dim, int32_t k);
int ihg_search_candidates(const float* features, int64_t ld, int32_t dim, int64_t query_row0, int64_t item_row0, int64_t n_items,
                          const float* item_bias, const int64_t* users, const int64_t* queries, const float* query_rows, int64_t ld_q, int32_t q_dim,
                          const uint32_t* item_mask, const int64_t* excl_ptr, const int32_t* excl_items, const int64_t* excl_row, int64_t n_excl_rows,
                          const int64_t* cand_ptr, const int32_t* cand_items, const int64_t* cand_row, int64_t n_cand_rows, int64_t total,
                          float lambda_muq, int64_t n_pairs, int32_t k, float* top_scores, int32_t* top_items, float* all_scores,
                          void* workspace, int64_t workspace_bytes, int32_t cosine, int32_t* passes, ihg_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * DEVICE: the attention of the GAT baseline over the pairwise graph (csrc/gat.hip).  Replaces GATLayer.forward after its transform
 * (Models/GnnLayers.py:98-115: the [nnz, 2, d] row gather, feature_aggregate, dgl.ops.edge_softmax and dgl.ops.u_mul_e_sum) and autograd's backward of it.
 * Graph: the symmetric CSR of the pairwise adjacency (ihg_build_pair_csr) - entry p of row v with column u = ids[p] is the edge u -> v, so row v lists
 * v's incoming edges; mirror[p] is the position of the reverse edge v -> u in row u.  Split-row plan as in ihg_node_segment_sum, plus seg_row[s] = the
 * row that segment s belongs to.  h [n_rows, dim] = feature_transform(x); weight = feature_aggregate.0.weight as a DEVICE vector ([w_src | w_dst], 2 dim
 * floats, for IHG_GAT_CONCAT; dim floats for IHG_GAT_PRODUCT), bias = feature_aggregate.0.bias (one DEVICE float); activation as Gs.Gnn.gat_activation
 * (Helpers/GlobalSettings.py:59-66).
 *   ihg_gat_attention_fwd  z[p] = act(w_src . h[u] + w_dst . h[v] + c)  (concat)  |  act(w . (h[u] * h[v]) + c)  (product)
 *                          alpha[p] = softmax of z over row v (max subtracted), alpha_mirror[mirror[p]] = alpha[p]      (all [nnz], caller-owned)
 *                          The layer output is then ihg_node_segment_sum(h, rowptr, ids, entry_scale = alpha): out[v] = sum_p alpha[p] h[u]; an empty row is zero.
 *   ihg_gat_scores_bwd     given dout [n_rows, dim]: ds[p] = alpha (dout[v] . h[u] - sum_row alpha (dout[v] . h[u'])) act'(z[p]) - the gradient of the
 *                          score before the activation (torch's conventions at 0) - and node_sums [n_rows, 2]: column 1 = sum of ds over row v (v as the
 *                          destination), column 0 (concat only) = sum of ds[mirror[q]] over row v (v as the source)
 *   ihg_gat_symmetrize     product: ds_sym[p] = ds[p] + ds[mirror[p]]
 *   ihg_gat_finish_bwd     dh [n_rows, dim] holds ihg_node_segment_sum(dout, entry_scale = alpha_mirror) on entry (the transposed aggregation); adds the score
 *                          terms: node_sums[v,0] w_src + node_sums[v,1] w_dst (concat) or w * b[v] with b = ihg_node_segment_sum(h, entry_scale = ds_sym)
 *                          (product; b unused for concat), and writes dweight (2 dim or dim floats) and dbias (1 float) as fixed-order column sums.
 * All four calls share one workspace of ihg_gat_workspace_bytes(n_rows, n_segments, dim, head) bytes.  No float atomics (bitwise reproducible), no [nnz, dim]
 * buffer, no synchronisation.  Any dim > 0; rows with dim % 4 == 0, 16-byte aligned, take the 16-B/lane path.
 */
#define IHG_GAT_CONCAT        0
#define IHG_GAT_PRODUCT       1
#define IHG_GAT_LEAKY_RELU    0   /* nn.LeakyReLU(), slope 0.01 */
#define IHG_GAT_RELU          1
#define IHG_GAT_TANH          2
int64_t ihg_gat_workspace_bytes(int64_t n_rows, int64_t n_segments, int32_t dim, int32_t head);
int ihg_gat_attention_fwd(const float* h, int64_t ld_h, const int32_t* rowptr, const int32_t* ids, const int32_t* mirror, const int32_t* row_order, int64_t n_rows,
                          int32_t dim, const float* weight, const float* bias, int32_t head, int32_t activation, int32_t heavy_threshold, const int32_t* seg_begin,
                          const int32_t* seg_end, const int32_t* seg_row, int64_t n_segments, const int32_t* heavy_rows, const int32_t* heavy_segptr, int64_t n_heavy,
                          float* z, float* alpha, float* alpha_mirror, void* workspace, int64_t workspace_bytes, ihg_stream_t stream);
int ihg_gat_scores_bwd(const float* h, int64_t ld_h, const float* dout, int64_t ld_dout, const int32_t* rowptr, const int32_t* ids, const int32_t* mirror,
                       const int32_t* row_order, int64_t n_rows, int32_t dim, int32_t head, int32_t activation, int32_t heavy_threshold, const int32_t* seg_begin,
                       const int32_t* seg_end, const int32_t* seg_row, int64_t n_segments, const int32_t* heavy_rows, const int32_t* heavy_segptr, int64_t n_heavy,
                       const float* z, const float* alpha, float* ds, float* node_sums, void* workspace, int64_t workspace_bytes, ihg_stream_t stream);
int ihg_gat_symmetrize(const float* ds, const int32_t* mirror, int64_t nnz, float* ds_sym, ihg_stream_t stream);
int ihg_gat_finish_bwd(const float* h, int64_t ld_h, const float* b, int64_t ld_b, const float* node_sums, const float* weight, int32_t head, int64_t n_rows,
                       int32_t dim, float* dh, int64_t ld_dh, float* dweight, float* dbias, void* workspace, int64_t workspace_bytes, ihg_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * DEVICE: the phase-2 attention of IHGNNLayer (csrc/phase2.hip).  Replaces fake_gat's forward after its transform (Models/GnnLayers.py:200-216, 227-230:
 * GATLayer.forward over the graph whose edges run hyperedge -> member node) and autograd's backward of it.
 * Graph: the layout's node-major CSR (ihg_build_csr) - entry p of row v with e = ids[p] is the edge e -> v, so row v lists v's hyperedges; pos[p] = 3 e + type(v)
 * is the entry's slot in an edge-major [n_edges, 3] table (a permutation of [0, 3 n_edges)); split-row plan and seg_row as in ihg_gat_attention_fwd.
 * h [n_rows, dim] and ef [n_edges, dim]: the node and hyperedge features after fake_gat.feature_transform; weight / bias / head / activation as in
 * ihg_gat_attention_fwd (concat: [w_src | w_dst], w_src meets ef, w_dst meets h).  edge_weight [n_edges] or NULL: the multiplicity m_e of a hyperedge kept once.
 *   ihg_phase2_attention_fwd  z[p] = act(w_src . ef[e] + w_dst . h[v] + c)  (concat)  |  act(w . (ef[e] * h[v]) + c)  (product)
 *                             alpha[p] = m_e exp(z[p] - max) / sum over row v of m exp(z - max),  alpha_edge[pos[p]] = alpha[p]      (all [3 n_edges], caller-owned)
 *                             The layer output is then ihg_node_segment_sum(ef, rowptr, ids, entry_scale = alpha); an empty row is zero.
 *   ihg_phase2_scores_bwd     given dout [n_rows, dim]: ds[p] = alpha (dout[v] . ef[e] - sum_row alpha (dout[v] . ef[e'])) act'(z[p]), ds_edge[pos[p]] = ds[p],
 *                             node_sums [n_rows, 2]: column 1 = sum of ds over row v (column 0 is not written)
 *   ihg_phase2_edges_bwd      edge-major, one [n_edges, dim] store: def[e] = sum_k alpha_edge[e, k] dout[i3[e, k]] + (sum_k ds_edge[e, k]) w_src  (concat)
 *                             | + w * sum_k ds_edge[e, k] h[i3[e, k]]  (product)
 *   ihg_phase2_finish_bwd     dh[v] = node_sums[v, 1] w_dst (concat) or w * b[v] with b = ihg_node_segment_sum(ef, entry_scale = ds) (product; b unused for
 *                             concat, ef and ds_edge unused for product); dweight (2 dim or dim floats) and dbias (1 float) as fixed-order column sums.
 *   ihg_phase2_add_rows       dst[r] += src[r] over [n_rows, dim] rows: the second contribution to a gradient that two passes of the layer's backward form
 * The calls share one workspace of ihg_phase2_workspace_bytes(...) bytes.  No float atomics (bitwise reproducible), no [3 n_edges, dim] buffer, no
 * synchronisation.  Any dim > 0; rows with dim % 4 == 0, 16-byte aligned, take the 16-B/lane path.
 */
int64_t ihg_phase2_workspace_bytes(int64_t n_rows, int64_t n_edges, int64_t n_segments, int32_t dim, int32_t head);
int ihg_phase2_attention_fwd(const float* h, int64_t ld_h, const float* ef, int64_t ld_ef, const int32_t* rowptr, const int32_t* ids, const int32_t* pos,
                             const int32_t* row_order, int64_t n_rows, int64_t n_edges, int32_t dim, const float* weight, const float* bias,
                             const float* edge_weight, int32_t head, int32_t activation, int32_t heavy_threshold, const int32_t* seg_begin, const int32_t* seg_end,
                             const int32_t* seg_row, int64_t n_segments, const int32_t* heavy_rows, const int32_t* heavy_segptr, int64_t n_heavy, float* z,
                             float* alpha, float* alpha_edge, void* workspace, int64_t workspace_bytes, ihg_stream_t stream);
int ihg_phase2_scores_bwd(const float* ef, int64_t ld_ef, const float* dout, int64_t ld_dout, const int32_t* rowptr, const int32_t* ids, const int32_t* pos,
                          const int32_t* row_order, int64_t n_rows, int64_t n_edges, int32_t dim, int32_t head, int32_t activation, int32_t heavy_threshold,
                          const int32_t* seg_begin, const int32_t* seg_end, const int32_t* seg_row, int64_t n_segments, const int32_t* heavy_rows,
                          const int32_t* heavy_segptr, int64_t n_heavy, const float* z, const float* alpha, float* ds, float* ds_edge, float* node_sums,
                          void* workspace, int64_t workspace_bytes, ihg_stream_t stream);
int ihg_phase2_edges_bwd(const float* dout, int64_t ld_dout, const float* h, int64_t ld_h, const int32_t* i3, const float* alpha_edge, const float* ds_edge,
                         const float* weight, int32_t head, int64_t n_edges, int32_t dim, float* def, int64_t ld_def, ihg_stream_t stream);
int ihg_phase2_finish_bwd(const float* h, int64_t ld_h, const float* ef, int64_t ld_ef, const float* b, int64_t ld_b, const float* node_sums, const float* ds_edge,
                          const float* weight, int32_t head, int64_t n_rows, int64_t n_edges, int32_t dim, float* dh, int64_t ld_dh, float* dweight, float* dbias,
                          void* workspace, int64_t workspace_bytes, ihg_stream_t stream);
int ihg_phase2_add_rows(float* dst, int64_t ld_dst, const float* src, int64_t ld_src, int64_t n_rows, int32_t dim, ihg_stream_t stream);

/* Small device-side helpers that keep a training step free of framework launches (torch fills / index ops of a few microseconds each):
 *   ihg_zero_floats      p[0 .. n) = 0
 *   ihg_mark_rows        mask[rows[k]] = value, k < n (rows as int64 OR int32: pass the other NULL) - the row mask of a sparse cotangent, set before
 *                        the pull that reads it and cleared after (ihg_node_segment_sum's src_mask)
 *   ihg_batch_node_rows  rows[0 .. 3 b) = users | queries + query_row0 | items + item_row0 (Models/RawGnn.py:128-131); rows32 (may be NULL): the same as int32
 *   ihg_zero_rows        base[rows[k], 0 .. dim) = 0, k < n
 */
int ihg_zero_floats(float* p, int64_t n, ihg_stream_t stream);
int ihg_mark_rows(const int64_t* rows64, const int32_t* rows32, int64_t n, uint8_t* mask, int32_t value, ihg_stream_t stream);
int ihg_batch_node_rows(const int64_t* users, const int64_t* queries, const int64_t* items, int64_t batch, int64_t query_row0, int64_t item_row0,
                        int64_t* rows, int32_t* rows32, ihg_stream_t stream);
int ihg_zero_rows(float* base, int64_t ld, int32_t dim, const int64_t* rows, int64_t n, ihg_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * DEVICE: the Srrl baseline (Models/Srrl.py, csrc/srrl.hip).  Every module of that model is one block
 *     F.normalize(cat(a, b), dim=-1) -> nn.Linear -> optional nn.LeakyReLU()          (Aggregation: one block; MLP: one block, then a plain Linear)
 *   ihg_cat_linear_fwd   out[r] = act(w n(cat(a[ia(r)], b[ib(r)])) + bias), r < n_rows.  A source is a row table (base, ld, width), an optional int64 index vector and a
 *                        repeat factor rep >= 1: row r reads table row idx[r / rep] (idx NULL: row r / rep) - the `expand` of a [B, 1, .] operand over k negatives, or one
 *                        user / query row over all items at evaluation.  n_rows must be whole groups of both repeat factors.  width_b == 0: a single source.
 *                        Index entries must name rows of their table: they are not checked.
 *                        n(x) = x / max(|x|_2, 1e-12) (F.normalize) when `normalize` != 0, else x.  activation: IHG_ACT_NONE or IHG_ACT_LEAKY_RELU (slope 0.01).
 *                        w [m, width_a + width_b] with row stride ld_w; out [n_rows, m] with any ld_out >= m.  With `normalize` the row's 1 / max(|x|, eps) goes to
 *                        inv_norm [n_rows] for the backward.  The scale is applied to the row's products after the sum (w (x / n) = (w x) / n).
 *   ihg_cat_linear_bwd   autograd's backward of the same block in one call: dz = dy * act'(y) formed as dy is loaded (act'(y) = y > 0 ? 1 : 0.01, no pre-activation stored),
 *                        dw [m, K] and dbias [m] (NULL: skipped) as per-workgroup partials added in a fixed order (no atomics, bitwise reproducible), and the input
 *                        gradient of F.normalize as autograd forms it - (dx^ - x^ (x^ . dx^)) / |x| above eps, dx^ / eps below (stored inverse norm = 1 / eps) - split
 *                        into da [n_rows / rep_a, width_a] and db [n_rows / rep_b, width_b], the rep rows of a group added in ascending order.  Either may be NULL.
 *                        These are ROW gradients: a gathered source lands in its table through ihg_batch_combine + ihg_batch_rows_add.
 *                        n_rows == 0: dw and dbias are zeroed.  workspace: ihg_cat_linear_workspace_bytes(n_rows, width_a + width_b, m) bytes, 16-byte aligned.
 *   Widths: width_a + width_b = 64 / 128 (d = 32 / 64) with both sources' rows and the weight's rows on 16-byte boundaries run on the matrix cores in exact fp32
 *   (v_mfma_f32_32x32x2_f32; the backward for m <= 128); every other width up to ihg_cat_linear_max_width() = 256, alignment or m: the any-width kernels, one thread
 *   per output element, rows staged in LDS 16 at a time, sums in index order.
 *   No allocation and no synchronisation inside the library.
 *   ihg_rows_dot_fwd     s[r] = sum_c x[r, c] y[r / rep, c]                                 (Models/Srrl.py:209, 221, 233 with their broadcast)
 *   ihg_rows_dot_bwd     dx[r] = ds[r] y[r / rep], dy[g] = sum_{r in g} ds[r] x[r] in ascending r; either NULL: skipped
 *   ihg_kg_loss          the KG loss of Helpers/TrainTestHelper.py:185-201 in one launch: pos [batch], neg [batch, k], weight [batch] or NULL (Gs.Srrl.uni_weight):
 *                        loss = (-sum w logsigmoid(pos) / sum w - sum w mean_k logsigmoid(-neg) / sum w) / 2, with dpos [batch] and dneg [batch, k]; fixed-order sums
 *   ihg_rows_topk        per row of a dense fp32 score matrix [n_rows, n_items] (row stride ld): the k <= 128 best (item, score) pairs, best first, equal scores in
 *                        ascending item id (ihg_score_topk's order); items [n_rows, k] int64, top_scores [n_rows, k]; beyond n_items entries: -1 / -inf.  A NaN is not ranked.
 */
#define IHG_ACT_NONE          0
#define IHG_ACT_LEAKY_RELU    3   /* nn.LeakyReLU(): the block kernels of the Srrl baseline only */
int32_t ihg_cat_linear_max_width(void);
int64_t ihg_cat_linear_workspace_bytes(int64_t n_rows, int32_t width, int32_t m);      /* -1: a width beyond ihg_cat_linear_max_width() */
int ihg_cat_linear_fwd(const float* a, int64_t ld_a, int32_t width_a, const int64_t* idx_a, int64_t rep_a, const float* b, int64_t ld_b, int32_t width_b, const int64_t* idx_b,
                       int64_t rep_b, const float* w, int64_t ld_w, const float* bias, int32_t m, int32_t normalize, int32_t activation, float* out, int64_t ld_out,
                       float* inv_norm, int64_t n_rows, ihg_stream_t stream);
int ihg_cat_linear_bwd(const float* dy, int64_t ld_dy, const float* y, int64_t ld_y, const float* a, int64_t ld_a, int32_t width_a, const int64_t* idx_a, int64_t rep_a,
                       const float* b, int64_t ld_b, int32_t width_b, const int64_t* idx_b, int64_t rep_b, const float* inv_norm, const float* w, int64_t ld_w, int32_t m,
                       int32_t normalize, int32_t activation, float* dw, int64_t ld_dw, float* dbias, float* da, int64_t ld_da, float* db, int64_t ld_db, int64_t n_rows,
                       void* workspace, int64_t workspace_bytes, ihg_stream_t stream);
int ihg_rows_dot_fwd(const float* x, int64_t ld_x, const float* y, int64_t ld_y, int64_t rep, float* s, int64_t n_rows, int32_t width, ihg_stream_t stream);
int ihg_rows_dot_bwd(const float* ds, const float* x, int64_t ld_x, const float* y, int64_t ld_y, int64_t rep, float* dx, int64_t ld_dx, float* dy, int64_t ld_dy, int64_t n_rows,
                     int32_t width, ihg_stream_t stream);
int ihg_kg_loss(const float* pos, const float* neg, int64_t ld_neg, const float* weight, int64_t batch, int32_t k, float* loss, float* dpos, float* dneg, int64_t ld_dneg,
                ihg_stream_t stream);
int ihg_rows_topk(const float* scores, int64_t ld, int64_t n_rows, int64_t n_items, int32_t k, int64_t* items, float* top_scores, ihg_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * DEVICE: the GRU query encoder (csrc/recurrent.hip; Gs.Query.transform == 'gru').  For bag q with word rows x_1 .. x_T of `table` in the order of `words`, h_0 = 0:
 *   r = sigmoid(W_ir x + b_ir + W_hr h + b_hr), z = sigmoid(W_iz x + b_iz + W_hz h + b_hz), n = tanh(W_in x + b_in + r * (W_hn h + b_hn)), h' = (1 - z) n + z h
 * (torch.nn.GRU: w_ih / w_hh [3 dim, dim] contiguous, b_ih / b_hh [3 dim], gate order r, z, n) and out[q] = h_T; an empty bag gives a zero row and no gradient.
 * fp32 throughout (v_mfma_f32_16x16x4_f32).  dim is 32, 64, 128 or 256: a caller with another width appends zero columns / rows to every operand, which is exact.
 * A workgroup owns 32 bags that are adjacent in `bag_order` (bags by decreasing length; NULL: as they are numbered) and runs its own time loop to its longest member: the
 * launch count does not depend on the bag lengths - one launch forwards, four backwards - and nothing synchronises; results do not depend on bag_order.
 *   ihg_gru_fwd   out [n_bags, dim] with any row stride ld_out >= dim and no alignment asked of it (a row block of X0, a column slice of the feature matrix).  `saved`
 *                 (ihg_gru_saved_bytes(n_words, dim) bytes, 16-byte aligned; NULL outside autograd: nothing is stored): r, z, n, W_hn h + b_hn and h_{t-1} of every
 *                 word occurrence - 5 n_words dim floats.  `workspace` is not read today (kept for an input projection hoisted to the vocabulary rows).
 *   ihg_gru_bwd   from the COMPLETE cotangent d_query [n_bags, dim] (any row stride): d_table [n_table_rows, dim] contiguous, every row written - the sum over the
 *                 word's positions in position order (word_ptr [n_table_rows + 1], word_pos [n_words]: ihg_node_segment_sum over the per-occurrence gradients) -,
 *                 dw_ih, dw_hh [3 dim, dim], db_ih, db_hh [3 dim]: summed over fixed slabs of occurrences and the slabs in slab order.  No float atomics: two runs
 *                 give the same bits.  `workspace`: ihg_gru_workspace_bytes(n_bags, n_words, dim) bytes, 16-byte aligned.
 * IHG_ERR_INVALID / IHG_ERR_WORKSPACE have launched nothing.  n_bags == 0 or n_words == 0: IHG_OK - the forward writes zero rows, the backward zeroes all five gradients.
 * The two *_bytes calls take any 1 <= dim <= 256 (the size at the next tiled width) and answer -1 beyond.
 */
int64_t ihg_gru_workspace_bytes(int64_t n_bags, int64_t n_words, int32_t dim);
int64_t ihg_gru_saved_bytes(int64_t n_words, int32_t dim);
int ihg_gru_fwd(const float* table, int64_t ld_table, const int32_t* bag_ptr, const int32_t* words, const int32_t* bag_order, int64_t n_bags, int64_t n_words,
                const float* w_ih, const float* w_hh, const float* b_ih, const float* b_hh, float* out, int64_t ld_out, float* saved, void* workspace,
                int64_t workspace_bytes, int32_t dim, ihg_stream_t stream);
int ihg_gru_bwd(const float* d_query, int64_t ld_dq, const float* table, int64_t ld_table, const int32_t* bag_ptr, const int32_t* words, const int32_t* bag_order,
                int64_t n_bags, int64_t n_words, const int32_t* word_ptr, const int32_t* word_pos, int64_t n_table_rows, const float* w_ih, const float* w_hh,
                const float* saved, float* d_table, float* dw_ih, float* dw_hh, float* db_ih, float* db_hh, void* workspace, int64_t workspace_bytes, int32_t dim,
                ihg_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* IHGNN_HIP_H */
