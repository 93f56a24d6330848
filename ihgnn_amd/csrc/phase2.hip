// phase2.hip - the phase-2 attention of IHGNNLayer (reference Models/GnnLayers.py:200-216, 227-230: GATLayer.forward, lines 96-115, over the "fake" graph whose
// edges run hyperedge -> member node).
//
// The graph is the layout's node_csr: entry p of row v with e = ids[p] is the edge e -> v, so row v lists v's hyperedges; pos[p] = 3 e + type(v) is the
// entry's slot in an edge-major [E, 3] table (every hyperedge has exactly one member of each type: a permutation of [0, 3 E)).  Two row tables instead of
// GAT's one: ef [E, d] (the sources) and h [N, d] (the destinations), both already through fake_gat.feature_transform.
//   forward   concat: one projection per ROW of each table (a[e] = w_src . ef[e], b[v] = w_dst . h[v]), scores are 4-byte gathers; product: a row
//             gather-dot per entry (attention.hpp).  Softmax per node row, written twice (alpha in list order, alpha_edge[pos[p]] = alpha[p]); then K7
//             (ihg_node_segment_sum over ef with entry_scale = alpha).
//   backward  d alpha[p] = dout[v] . ef[e] (row gather-dot), the softmax backward of attention.hpp (ds in list order, S[v] = sum over row v of ds), ds
//             scattered to ds_edge[pos[p]]; d ef by ONE edge-major pass (a lane group owns hyperedges: 3 row gathers of dout - 6 with the product head -, one
//             [E, d] store); d h = S[v] w_dst (concat) or w * K7(ef, entry_scale = ds)[v] (product); parameter gradients as fixed-order column sums.
// A layout that keeps identical triples once (mult[e] = m_e) stands for m_e copies of hyperedge e with identical scores - log m_e added to the logit:
// alpha[p] = m_e exp(z - max) / sum m exp(z - max); everything downstream is unchanged (d ef of a kept-once row is the sum over its copies).
// Split rows as in gat.hip: per segment, merged per row in a fixed tree.  No float atomics, bitwise-identical results run to run, no [3 E, d] tensor, no
// host synchronisation.
// The projection, the softmax (its multiplicity a template parameter), the gather-dot, the softmax backward and the node-row gradient are attention.hpp's,
// shared with gat.hip; what is phase 2's own is below: the copy of ds to its edge-major slots, the edge-major backward, the column sums and the row add.
#include "attention.hpp"

namespace {

// ds_edge[pos[p]] = ds[p]: the score gradients at their slots of the edge-major table
__global__ __launch_bounds__(kBlockThreads) void p2_to_edge_slots_kernel(const float* __restrict__ ds, const int32_t* __restrict__ pos, int64_t nnz,
                                                                         float* __restrict__ ds_edge) {
    for (int64_t p = static_cast<int64_t>(blockIdx.x) * kBlockThreads + threadIdx.x; p < nnz; p += static_cast<int64_t>(gridDim.x) * kBlockThreads)
        ds_edge[pos[p]] = ds[p];
}

// Edge-major (K5's shape: G lanes own a hyperedge, no atomics):
//   def[e] = sum_k alpha_edge[e, k] dout[i3[e, k]]  +  (sum_k ds_edge[e, k]) w_src  (concat)  |  w * sum_k ds_edge[e, k] h[i3[e, k]]  (product)
template <int VEC, int G, bool PRODUCT>
__global__ __launch_bounds__(kBlockThreads) void p2_edges_bwd_kernel(const float* __restrict__ dout, int64_t ld_dout, const float* __restrict__ h, int64_t ld_h,
                                                                     const int32_t* __restrict__ i3, const float* __restrict__ alpha_edge,
                                                                     const float* __restrict__ ds_edge, const float* __restrict__ w, int64_t n_edges, int dim_vec,
                                                                     float* __restrict__ def, int64_t ld_def) {
    constexpr int GPW = kWave / G;
    const int lane = threadIdx.x & (kWave - 1);
    const int lig = lane & (G - 1);
    const int grp = lane / G;
    for (int64_t e0 = global_wave_id() * GPW; e0 < n_edges; e0 += global_wave_count() * GPW) {
        const int64_t e = e0 + grp;
        if (e >= n_edges) continue;
        int64_t id[3];
        float al[3], s[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            id[k] = i3[3 * e + k];
            al[k] = alpha_edge[3 * e + k];
            s[k] = ds_edge[3 * e + k];
        }
        const float s_sum = (s[0] + s[1]) + s[2];
        for (int c = lig; c < dim_vec; c += G) {
            Frag<VEC> row[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) row[k] = Frag<VEC>::load(dout + id[k] * ld_dout + c * VEC);
            Frag<VEC> acc = Frag<VEC>::zero();
#pragma unroll
            for (int k = 0; k < 3; ++k) acc.add_scaled(row[k], al[k]);
            if (PRODUCT) {
#pragma unroll
                for (int k = 0; k < 3; ++k) row[k] = Frag<VEC>::load(h + id[k] * ld_h + c * VEC);
                Frag<VEC> t = Frag<VEC>::zero();
#pragma unroll
                for (int k = 0; k < 3; ++k) t.add_scaled(row[k], s[k]);
                acc.add(frag_mul(Frag<VEC>::load(w + c * VEC), t));
            } else {
                acc.add_scaled(Frag<VEC>::load(w + c * VEC), s_sum);
            }
            acc.store(def + e * ld_def + c * VEC);
        }
    }
}

// Parameter gradients: column sums over the rows of a table, kParamRows rows per workgroup, then the workgroups' partials in a fixed tree.
//   y == NULL: column c < dim sums s(r) x[r, c], column dim (when n_cols = dim + 1) sums s(r), with s(r) = s[r stride] + ... + s[r stride + TERMS - 1]
//   y != NULL: column c < dim sums x[r, c] y[r, c], column dim as above
// cw (a power of two <= kBlockThreads) threads stand side by side on a row; the kBlockThreads / cw row slices of a workgroup walk every slices-th row and are
// added in slice order.
template <int TERMS>
__global__ __launch_bounds__(kBlockThreads) void p2_colsum_partials_kernel(const float* __restrict__ x, int64_t ld_x, const float* __restrict__ y, int64_t ld_y,
                                                                             const float* __restrict__ s, int s_stride, int64_t n_rows, int dim, int n_cols, int cw,
                                                                             float* __restrict__ partials) {
    __shared__ float red[kBlockThreads];
    const int slices = kBlockThreads / cw;
    const int sl = threadIdx.x / cw, lc = threadIdx.x & (cw - 1);
    const int64_t r0 = static_cast<int64_t>(blockIdx.x) * kParamRows;
    const int64_t r1 = r0 + kParamRows < n_rows ? r0 + kParamRows : n_rows;
    for (int c0 = 0; c0 < n_cols; c0 += cw) {                            // (uniform over the workgroup: the barriers below are met by every thread)
        const int c = c0 + lc;
        float acc = 0.f;
        // (the loads of several rows in flight per thread; the adds stay in row order)
        if (c < dim && y != nullptr) {
#pragma unroll 8
            for (int64_t r = r0 + sl; r < r1; r += slices) acc += x[r * ld_x + c] * y[r * ld_y + c];
        } else if (c < n_cols) {
#pragma unroll 8
            for (int64_t r = r0 + sl; r < r1; r += slices) {
                float sr = s[r * s_stride];
#pragma unroll
                for (int t = 1; t < TERMS; ++t) sr += s[r * s_stride + t];
                acc += c < dim ? sr * x[r * ld_x + c] : sr;
            }
        }
        red[threadIdx.x] = acc;
        __syncthreads();
        if (sl == 0 && c < n_cols) {
            float total = red[lc];
            for (int k = 1; k < slices; ++k) total += red[k * cw + lc];
            partials[static_cast<int64_t>(blockIdx.x) * n_cols + c] = total;
        }
        __syncthreads();
    }
}

// columns [0, n_weight_cols) -> dweight, a further column -> dbias[0]; one workgroup per column adds the workgroups' partials in a fixed tree
__global__ __launch_bounds__(kBlockThreads) void p2_colsum_finish_kernel(const float* __restrict__ partials, int64_t n_blocks, int n_cols, int n_weight_cols,
                                                                           float* __restrict__ dweight, float* __restrict__ dbias) {
    __shared__ float red[kBlockThreads];
    const int c = blockIdx.x;
    float acc = 0.f;
    for (int64_t k = threadIdx.x; k < n_blocks; k += kBlockThreads) acc += partials[k * n_cols + c];
    acc = block_sum(acc, red);
    if (threadIdx.x == 0) {
        if (c < n_weight_cols) dweight[c] = acc;
        else dbias[0] = acc;
    }
}

// dst[r] += src[r]: the second contribution to a gradient that two passes of the layer's backward form (fake_gat's transform runs on the node rows AND the
// hyperedge rows; the node features feed the interactor AND the transform) - in the library, so that a step stays free of framework launches
__global__ __launch_bounds__(kBlockThreads) void p2_add_rows_kernel(float* __restrict__ dst, int64_t ld_dst, const float* __restrict__ src, int64_t ld_src,
                                                                    int64_t n_rows, int dim) {
    const int64_t total = n_rows * dim;
    for (int64_t i = static_cast<int64_t>(blockIdx.x) * kBlockThreads + threadIdx.x; i < total; i += static_cast<int64_t>(gridDim.x) * kBlockThreads) {
        const int64_t r = i / dim;
        const int c = static_cast<int>(i - r * dim);
        dst[r * ld_dst + c] += src[r * ld_src + c];
    }
}

// a layout without multiplicities (mult == NULL) runs the instances that read none
template <bool CONCAT>
void launch_p2_softmax(const float* a, const float* b, const float* bias, const float* mult, int act, const Plan& pl, float* z, float* alpha, float* alpha_edge,
                       float* partials, hipStream_t s) {
    if (mult != nullptr) launch_softmax<CONCAT, true>(a, b, bias, mult, act, pl, z, alpha, alpha_edge, partials, s);
    else launch_softmax<CONCAT, false>(a, b, bias, nullptr, act, pl, z, alpha, alpha_edge, partials, s);
}

void launch_edges_bwd(bool vec4, bool product, const float* dout, int64_t ld_dout, const float* h, int64_t ld_h, const int32_t* i3, const float* alpha_edge,
                      const float* ds_edge, const float* w, int64_t n_edges, int dim, float* def, int64_t ld_def, hipStream_t st) {
    with_row_lanes(vec4, dim, [&](auto vec, auto g) {
        constexpr int VEC = decltype(vec)::value, G = decltype(g)::value;
        const dim3 grid(group_grid(n_edges, G)), block(kBlockThreads);
        if (product)
            hipLaunchKernelGGL((p2_edges_bwd_kernel<VEC, G, true>), grid, block, 0, st, dout, ld_dout, h, ld_h, i3, alpha_edge, ds_edge, w, n_edges, dim / VEC, def, ld_def);
        else
            hipLaunchKernelGGL((p2_edges_bwd_kernel<VEC, G, false>), grid, block, 0, st, dout, ld_dout, h, ld_h, i3, alpha_edge, ds_edge, w, n_edges, dim / VEC, def, ld_def);
    });
}

// One column sum into dweight[0 .. dim) (and, with_bias, the further column into dbias[0]) over n_rows rows; partials: param_blocks(n_rows) * n_cols floats
template <int TERMS>
void launch_colsum(const float* x, int64_t ld_x, const float* y, int64_t ld_y, const float* s, int s_stride, int64_t n_rows, int dim, bool with_bias,
                   float* partials, float* dweight, float* dbias, hipStream_t st) {
    const int n_cols = dim + (with_bias ? 1 : 0);
    const int64_t blocks = param_blocks(n_rows);
    int cw = 4;                                                          // over dim, at most a workgroup: the bias column joins the last pass or gets one of its own
    while (cw < dim && cw < kBlockThreads) cw <<= 1;
    hipLaunchKernelGGL(p2_colsum_partials_kernel<TERMS>, dim3(static_cast<unsigned>(blocks)), dim3(kBlockThreads), 0, st, x, ld_x, y, ld_y, s, s_stride, n_rows, dim, n_cols,
                       cw, partials);
    hipLaunchKernelGGL(p2_colsum_finish_kernel, dim3(n_cols), dim3(kBlockThreads), 0, st, partials, blocks, n_cols, dim, dweight, dbias);
}

}  // namespace

extern "C" {

int64_t ihg_phase2_workspace_bytes(int64_t n_rows, int64_t n_edges, int64_t n_segments, int32_t dim, int32_t head) {
    if (n_rows < 0 || n_edges < 0 || n_segments < 0 || dim <= 0) return -1;
    const int64_t fwd = (head == IHG_GAT_CONCAT ? n_rows + n_edges : 0) + 2 * n_segments;
    const int64_t bwd = n_segments;
    const int64_t params = param_blocks(n_rows) * (static_cast<int64_t>(dim) + 1) + (head == IHG_GAT_CONCAT ? param_blocks(n_edges) * dim : 0);
    return 4 * std::max<int64_t>(16, std::max(fwd, std::max(bwd, params)));
}

int ihg_phase2_attention_fwd(const float* h, int64_t ld_h, const float* ef, int64_t ld_ef, const int32_t* rowptr, const int32_t* ids, const int32_t* pos,
                             const int32_t* row_order, int64_t n_rows, int64_t n_edges, int32_t dim, const float* weight, const float* bias,
                             const float* edge_weight, int32_t head, int32_t activation, int32_t heavy_threshold, const int32_t* seg_begin, const int32_t* seg_end,
                             const int32_t* seg_row, int64_t n_segments, const int32_t* heavy_rows, const int32_t* heavy_segptr, int64_t n_heavy, float* z,
                             float* alpha, float* alpha_edge, void* workspace, int64_t workspace_bytes, ihg_stream_t stream) {
    const char* const what = "ihg_phase2_attention_fwd";
    const Plan pl = make_plan(rowptr, ids, pos, row_order, n_rows, heavy_threshold, seg_begin, seg_end, seg_row, n_segments, heavy_rows, heavy_segptr, n_heavy);
    if (const int rc = check_plan(what, pl, head, activation, dim); rc != IHG_OK) return rc;
    if (n_edges < 0 || ld_h < dim || ld_ef < dim) return fail(IHG_ERR_INVALID, "%s: bad size or row stride", what);
    if (n_rows == 0 || n_edges == 0) return IHG_OK;
    if (const int rc = check_pointers(what, {h, ef, weight, bias, z, alpha, alpha_edge, workspace}); rc != IHG_OK) return rc;
    if (const int rc = check_workspace(what, workspace_bytes, ihg_phase2_workspace_bytes(n_rows, n_edges, pl.n_segments, dim, head)); rc != IHG_OK) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    float* ws = static_cast<float*>(workspace);
    if (head == IHG_GAT_CONCAT) {
        float* a = ws;                                                   // [n_edges]
        float* b = a + n_edges;                                          // [n_rows]
        float* partials = b + n_rows;                                    // [n_segments, 2]
        launch_project<1>(rows16(dim, ld_ef, ef) && aligned16(weight), ef, ld_ef, weight, dim, n_edges, a, s);
        launch_project<1>(rows16(dim, ld_h, h) && aligned16(weight), h, ld_h, weight + dim, dim, n_rows, b, s);
        launch_p2_softmax<true>(a, b, bias, edge_weight, activation, pl, z, alpha, alpha_edge, partials, s);
    } else {
        // z[p] = act(w . (h[v] * ef[e]) + c)
        launch_row_dot(rows16(dim, ld_h, h) && rows16(dim, ld_ef, ef) && aligned16(weight), h, ld_h, weight, ef, ld_ef, bias, activation, pl, dim, z, s);
        launch_p2_softmax<false>(nullptr, nullptr, bias, edge_weight, activation, pl, z, alpha, alpha_edge, ws, s);
    }
    return check_launch(what);
}

int ihg_phase2_scores_bwd(const float* ef, int64_t ld_ef, const float* dout, int64_t ld_dout, const int32_t* rowptr, const int32_t* ids, const int32_t* pos,
                          const int32_t* row_order, int64_t n_rows, int64_t n_edges, int32_t dim, int32_t head, int32_t activation, int32_t heavy_threshold,
                          const int32_t* seg_begin, const int32_t* seg_end, const int32_t* seg_row, int64_t n_segments, const int32_t* heavy_rows,
                          const int32_t* heavy_segptr, int64_t n_heavy, const float* z, const float* alpha, float* ds, float* ds_edge, float* node_sums,
                          void* workspace, int64_t workspace_bytes, ihg_stream_t stream) {
    const char* const what = "ihg_phase2_scores_bwd";
    const Plan pl = make_plan(rowptr, ids, pos, row_order, n_rows, heavy_threshold, seg_begin, seg_end, seg_row, n_segments, heavy_rows, heavy_segptr, n_heavy);
    if (const int rc = check_plan(what, pl, head, activation, dim); rc != IHG_OK) return rc;
    if (n_edges < 0 || ld_ef < dim || ld_dout < dim) return fail(IHG_ERR_INVALID, "%s: bad size or row stride", what);
    if (n_rows == 0 || n_edges == 0) return IHG_OK;
    if (const int rc = check_pointers(what, {ef, dout, z, alpha, ds, ds_edge, node_sums, workspace}); rc != IHG_OK) return rc;
    if (const int rc = check_workspace(what, workspace_bytes, ihg_phase2_workspace_bytes(n_rows, n_edges, pl.n_segments, dim, head)); rc != IHG_OK) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    float* partials = static_cast<float*>(workspace);                     // [n_segments]
    // d alpha[p] = dout[v] . ef[e]
    launch_row_dot(rows16(dim, ld_ef, ef) && rows16(dim, ld_dout, dout), dout, ld_dout, nullptr, ef, ld_ef, nullptr, -1, pl, dim, ds, s);
    launch_softmax_bwd(z, alpha, ds, activation, pl, node_sums, partials, s);
    hipLaunchKernelGGL(p2_to_edge_slots_kernel, dim3(flat_grid(3 * n_edges)), dim3(kBlockThreads), 0, s, ds, pos, 3 * n_edges, ds_edge);
    return check_launch(what);
}

int ihg_phase2_edges_bwd(const float* dout, int64_t ld_dout, const float* h, int64_t ld_h, const int32_t* i3, const float* alpha_edge, const float* ds_edge,
                         const float* weight, int32_t head, int64_t n_edges, int32_t dim, float* def, int64_t ld_def, ihg_stream_t stream) {
    const char* const what = "ihg_phase2_edges_bwd";
    if (n_edges < 0 || dim <= 0 || ld_dout < dim || ld_h < dim || ld_def < dim) return fail(IHG_ERR_INVALID, "%s: bad size (edges=%lld dim=%d)", what, (long long)n_edges, dim);
    if (const int rc = check_head(what, head); rc != IHG_OK) return rc;
    if (n_edges == 0) return IHG_OK;
    if (const int rc = check_pointers(what, {dout, h, i3, alpha_edge, ds_edge, weight, def}); rc != IHG_OK) return rc;
    launch_edges_bwd(rows16(dim, ld_dout, dout) && rows16(dim, ld_h, h) && rows16(dim, ld_def, def) && aligned16(weight), head == IHG_GAT_PRODUCT, dout, ld_dout, h, ld_h,
                     i3, alpha_edge, ds_edge, weight, n_edges, dim, def, ld_def, static_cast<hipStream_t>(stream));
    return check_launch(what);
}

int ihg_phase2_finish_bwd(const float* h, int64_t ld_h, const float* ef, int64_t ld_ef, const float* b, int64_t ld_b, const float* node_sums, const float* ds_edge,
                          const float* weight, int32_t head, int64_t n_rows, int64_t n_edges, int32_t dim, float* dh, int64_t ld_dh, float* dweight, float* dbias,
                          void* workspace, int64_t workspace_bytes, ihg_stream_t stream) {
    const char* const what = "ihg_phase2_finish_bwd";
    const bool concat = head == IHG_GAT_CONCAT;
    if (n_rows < 0 || n_edges < 0 || dim <= 0 || ld_h < dim || ld_dh < dim || (head == IHG_GAT_PRODUCT && ld_b < dim) || (concat && ld_ef < dim))
        return fail(IHG_ERR_INVALID, "%s: bad size (rows=%lld edges=%lld dim=%d)", what, (long long)n_rows, (long long)n_edges, dim);
    if (const int rc = check_head(what, head); rc != IHG_OK) return rc;
    if (const int rc = check_pointers(what, {dweight, dbias, weight, workspace}); rc != IHG_OK) return rc;
    if (const int rc = check_workspace(what, workspace_bytes, ihg_phase2_workspace_bytes(n_rows, n_edges, 0, dim, head)); rc != IHG_OK) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (n_rows == 0 || n_edges == 0) {
        launch_zero_floats(dweight, concat ? 2 * dim : dim, s);
        launch_zero_floats(dbias, 1, s);
        return check_launch(what);
    }
    if (const int rc = check_pointers(what, {h, node_sums, dh}); rc != IHG_OK) return rc;
    if (concat ? (ef == nullptr || ds_edge == nullptr) : b == nullptr) return fail(IHG_ERR_INVALID, "%s: null pointer", what);
    float* node_partials = static_cast<float*>(workspace);
    float* edge_partials = node_partials + param_blocks(n_rows) * (dim + 1);
    if (concat) {
        // dw_src = sum_e (sum_k ds_edge[e, k]) ef[e]   |   dw_dst = sum_v S[v] h[v],  dc = sum_v S[v]
        launch_colsum<3>(ef, ld_ef, nullptr, 0, ds_edge, 3, n_edges, dim, false, edge_partials, dweight, dbias, s);
        launch_colsum<1>(h, ld_h, nullptr, 0, node_sums + 1, 2, n_rows, dim, true, node_partials, dweight + dim, dbias, s);
    } else {
        // dw = sum_v h[v] * b[v]   (b = K7(ef, entry_scale = ds)),  dc = sum_v S[v]
        launch_colsum<1>(h, ld_h, b, ld_b, node_sums + 1, 2, n_rows, dim, true, node_partials, dweight, dbias, s);
    }
    launch_node_grad<false, false>(rows16(dim, ld_dh, dh) && aligned16(weight) && (concat || rows16(dim, ld_b, b)), dh, ld_dh, b, ld_b, node_sums, weight, head, n_rows,
                                   dim, s);
    return check_launch(what);
}

int ihg_phase2_add_rows(float* dst, int64_t ld_dst, const float* src, int64_t ld_src, int64_t n_rows, int32_t dim, ihg_stream_t stream) {
    if (n_rows < 0 || dim <= 0 || ld_dst < dim || ld_src < dim) return fail(IHG_ERR_INVALID, "ihg_phase2_add_rows: bad size (rows=%lld dim=%d)", (long long)n_rows, dim);
    if (n_rows == 0) return IHG_OK;
    if (const int rc = check_pointers("ihg_phase2_add_rows", {dst, src}); rc != IHG_OK) return rc;
    hipLaunchKernelGGL(p2_add_rows_kernel, dim3(flat_grid(n_rows * dim)), dim3(kBlockThreads), 0, static_cast<hipStream_t>(stream), dst, ld_dst, src, ld_src, n_rows, dim);
    return check_launch("ihg_phase2_add_rows");
}

}  // extern "C"
