// gat.hip - the attention of the GAT baseline (reference Models/GnnLayers.py:48-115) over the symmetric CSR of the pairwise graph.
//
// Entry p of CSR row v with column u = ids[p] is the edge u -> v: row v lists v's incoming edges (the graph is symmetric, Dataset.py:86-88), and
// mirror[p] is the position of the reverse edge v -> u in row u.  The reference materialises [nnz, 2, d] rows (GnnLayers.py:100-107); here:
//   forward   scores z[p] (concat: two projections per NODE, gathered as 4-byte scalars; product: a row gather-dot per entry), a softmax over every
//             row written twice (alpha in list order, alpha_mirror[mirror[p]] = alpha[p]), then K7 (ihg_node_segment_sum with entry_scale = alpha)
//   backward  d alpha[p] = dout[v] . h[u] (row gather-dot), ds[p] = alpha (d alpha - sum_row alpha d alpha) act'(z), per-node sums of ds in both
//             directions (concat) or ds + ds[mirror] (product), then K7 over dout with alpha_mirror (and over h with ds + ds[mirror]) and the
//             fixed-order column sums of the parameter gradients.
// Rows longer than the split-row threshold are cut into the segments of the K7 plan: every per-row reduction (max and denominator of the softmax,
// the sum of alpha d alpha, the row sums of ds) is formed per segment and merged per row in a fixed tree by one workgroup - no float atomics,
// bitwise-identical results run to run.  No [nnz, d] tensor, no host synchronisation.
// The projection, the softmax, the gather-dot, the softmax backward and the node-row gradient are attention.hpp's, shared with phase2.hip; what is GAT's own
// is below: the per-node sums of ds over the edges a node is the source of, ds + ds[mirror], and the column sums of its parameter gradients (one thread per
// column; phase2.hip's column sums are the candidate to replace them once timed against these).
#include "attention.hpp"

namespace {

// concat: node_sums[2 v] = sum over row v of ds[mirror[q]] - the edges v -> u, where v is the SOURCE
__global__ __launch_bounds__(kBlockThreads) void gat_source_sums_kernel(const float* __restrict__ ds, Plan pl, float* __restrict__ node_sums, float* __restrict__ partials) {
    constexpr int G = kScalarLanes, GPW = kWave / G;
    const int lane = threadIdx.x & (kWave - 1);
    const int lig = lane & (G - 1);
    const int grp = lane / G;
    const int64_t n_units = pl.n_segments + pl.n_rows;
    for (int64_t u0 = global_wave_id() * GPW; u0 < n_units; u0 += global_wave_count() * GPW) {
        const Unit un = unit_at(pl, u0 + grp);
        float acc = 0.f;
        for (int i = lig; i < un.len; i += G) acc += ds[pl.mirror[un.begin + i]];
        acc = group_sum<G>(acc);
        if (lig == 0) {
            if (un.seg >= 0) partials[un.seg] = acc;
            else if (un.row >= 0) node_sums[2 * un.row] = acc;
        }
    }
}

__global__ __launch_bounds__(kBlockThreads) void gat_source_sums_finish_kernel(Plan pl, float* __restrict__ node_sums, const float* __restrict__ partials) {
    __shared__ float red[kBlockThreads];
    const int t = threadIdx.x;
    for (int64_t hr = blockIdx.x; hr < pl.n_heavy; hr += gridDim.x) {
        const int s0 = pl.heavy_segptr[hr], s1 = pl.heavy_segptr[hr + 1];
        float acc = 0.f;
        for (int sg = s0 + t; sg < s1; sg += kBlockThreads) acc += partials[sg];
        acc = block_sum(acc, red);
        if (t == 0) node_sums[2 * static_cast<int64_t>(pl.heavy_rows[hr])] = acc;
    }
}

// product: sym[p] = ds[p] + ds[mirror[p]] - both ends of every edge take w * h of the other end
__global__ __launch_bounds__(kBlockThreads) void gat_symmetrize_kernel(const float* __restrict__ ds, const int32_t* __restrict__ mirror, int64_t nnz, float* __restrict__ sym) {
    for (int64_t p = static_cast<int64_t>(blockIdx.x) * kBlockThreads + threadIdx.x; p < nnz; p += static_cast<int64_t>(gridDim.x) * kBlockThreads)
        sym[p] = ds[p] + ds[mirror[p]];
}

// Parameter gradients as column sums over the node rows, kParamRows rows per workgroup, then the workgroups' partials in index order.
//   concat: columns [0, d) sum node_sums[2 v] h[v], [d, 2 d) node_sums[2 v + 1] h[v], column 2 d node_sums[2 v + 1]   (dw_src | dw_dst | dc)
//   product: columns [0, d) sum h[v] * b[v] (twice dw: every edge is met from both ends), column d node_sums[2 v + 1]   (dw | dc)
__global__ __launch_bounds__(kBlockThreads) void gat_param_partials_kernel(const float* __restrict__ h, int64_t ld_h, const float* __restrict__ b, int64_t ld_b,
                                                                           const float* __restrict__ node_sums, int head, int64_t n_rows, int dim, int n_cols,
                                                                           float* __restrict__ partials) {
    const int64_t r0 = static_cast<int64_t>(blockIdx.x) * kParamRows;
    const int64_t r1 = r0 + kParamRows < n_rows ? r0 + kParamRows : n_rows;
    for (int c = threadIdx.x; c < n_cols; c += kBlockThreads) {
        float acc = 0.f;
        if (c == n_cols - 1) {
            for (int64_t r = r0; r < r1; ++r) acc += node_sums[2 * r + 1];
        } else if (head == IHG_GAT_CONCAT) {
            const int side = c >= dim ? 1 : 0;
            const int k = c - side * dim;
            for (int64_t r = r0; r < r1; ++r) acc += node_sums[2 * r + side] * h[r * ld_h + k];
        } else {
            for (int64_t r = r0; r < r1; ++r) acc += h[r * ld_h + c] * b[r * ld_b + c];
        }
        partials[static_cast<int64_t>(blockIdx.x) * n_cols + c] = acc;
    }
}

__global__ __launch_bounds__(kBlockThreads) void gat_param_finish_kernel(const float* __restrict__ partials, int64_t n_blocks, int n_cols, float weight_factor,
                                                                         float* __restrict__ dweight, float* __restrict__ dbias) {
    const int c = blockIdx.x * kBlockThreads + threadIdx.x;
    if (c >= n_cols) return;
    float acc = 0.f;
    for (int64_t k = 0; k < n_blocks; ++k) acc += partials[k * n_cols + c];
    if (c == n_cols - 1) dbias[0] = acc;
    else dweight[c] = acc * weight_factor;
}

}  // namespace

extern "C" {

int64_t ihg_gat_workspace_bytes(int64_t n_rows, int64_t n_segments, int32_t dim, int32_t head) {
    if (n_rows < 0 || n_segments < 0 || dim <= 0) return -1;
    const int64_t fwd = (head == IHG_GAT_CONCAT ? 2 * n_rows : 0) + 2 * n_segments;
    const int64_t bwd = n_segments;
    const int64_t n_cols = (head == IHG_GAT_CONCAT ? 2 * static_cast<int64_t>(dim) : dim) + 1;
    const int64_t params = param_blocks(n_rows) * n_cols;
    return 4 * std::max<int64_t>(16, std::max(fwd, std::max(bwd, params)));
}

int ihg_gat_attention_fwd(const float* h, int64_t ld_h, const int32_t* rowptr, const int32_t* ids, const int32_t* mirror, const int32_t* row_order, int64_t n_rows,
                          int32_t dim, const float* weight, const float* bias, int32_t head, int32_t activation, int32_t heavy_threshold, const int32_t* seg_begin,
                          const int32_t* seg_end, const int32_t* seg_row, int64_t n_segments, const int32_t* heavy_rows, const int32_t* heavy_segptr, int64_t n_heavy,
                          float* z, float* alpha, float* alpha_mirror, void* workspace, int64_t workspace_bytes, ihg_stream_t stream) {
    const char* const what = "ihg_gat_attention_fwd";
    const Plan pl = make_plan(rowptr, ids, mirror, row_order, n_rows, heavy_threshold, seg_begin, seg_end, seg_row, n_segments, heavy_rows, heavy_segptr, n_heavy);
    if (const int rc = check_plan(what, pl, head, activation, dim); rc != IHG_OK) return rc;
    if (ld_h < dim) return fail(IHG_ERR_INVALID, "%s: ld_h %lld < dim %d", what, (long long)ld_h, dim);
    if (n_rows == 0) return IHG_OK;
    if (const int rc = check_pointers(what, {h, weight, bias, z, alpha, alpha_mirror, workspace}); rc != IHG_OK) return rc;
    if (const int rc = check_workspace(what, workspace_bytes, ihg_gat_workspace_bytes(n_rows, pl.n_segments, dim, head)); rc != IHG_OK) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    float* ws = static_cast<float*>(workspace);
    const bool vec4 = rows16(dim, ld_h, h) && aligned16(weight);
    if (head == IHG_GAT_CONCAT) {
        // s[v] = (h[v] . w_src, h[v] . w_dst) once per node (GnnLayers.py:104, 111: w . [h_u | h_v] splits into two node terms)
        float* partials = ws + 2 * n_rows;                               // [n_segments, 2]
        launch_project<2>(vec4, h, ld_h, weight, dim, n_rows, ws, s);
        launch_softmax<true, false, 2>(ws, ws + 1, bias, nullptr, activation, pl, z, alpha, alpha_mirror, partials, s);
    } else {
        launch_row_dot(vec4, h, ld_h, weight, h, ld_h, bias, activation, pl, dim, z, s);
        launch_softmax<false, false>(nullptr, nullptr, bias, nullptr, activation, pl, z, alpha, alpha_mirror, ws, s);
    }
    return check_launch(what);
}

int ihg_gat_scores_bwd(const float* h, int64_t ld_h, const float* dout, int64_t ld_dout, const int32_t* rowptr, const int32_t* ids, const int32_t* mirror,
                       const int32_t* row_order, int64_t n_rows, int32_t dim, int32_t head, int32_t activation, int32_t heavy_threshold, const int32_t* seg_begin,
                       const int32_t* seg_end, const int32_t* seg_row, int64_t n_segments, const int32_t* heavy_rows, const int32_t* heavy_segptr, int64_t n_heavy,
                       const float* z, const float* alpha, float* ds, float* node_sums, void* workspace, int64_t workspace_bytes, ihg_stream_t stream) {
    const char* const what = "ihg_gat_scores_bwd";
    const Plan pl = make_plan(rowptr, ids, mirror, row_order, n_rows, heavy_threshold, seg_begin, seg_end, seg_row, n_segments, heavy_rows, heavy_segptr, n_heavy);
    if (const int rc = check_plan(what, pl, head, activation, dim); rc != IHG_OK) return rc;
    if (ld_h < dim || ld_dout < dim) return fail(IHG_ERR_INVALID, "%s: bad row stride", what);
    if (n_rows == 0) return IHG_OK;
    if (const int rc = check_pointers(what, {h, dout, z, alpha, ds, node_sums, workspace}); rc != IHG_OK) return rc;
    if (const int rc = check_workspace(what, workspace_bytes, ihg_gat_workspace_bytes(n_rows, pl.n_segments, dim, head)); rc != IHG_OK) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    float* partials = static_cast<float*>(workspace);                     // [n_segments]
    // d alpha[p] = dout[v] . h[u]   (u_mul_e_sum's gradient with respect to the edge weight, GnnLayers.py:114)
    launch_row_dot(rows16(dim, ld_h, h) && rows16(dim, ld_dout, dout), dout, ld_dout, nullptr, h, ld_h, nullptr, -1, pl, dim, ds, s);
    launch_softmax_bwd(z, alpha, ds, activation, pl, node_sums, partials, s);
    if (head == IHG_GAT_CONCAT) {
        hipLaunchKernelGGL(gat_source_sums_kernel, dim3(scalar_grid(pl)), dim3(kBlockThreads), 0, s, ds, pl, node_sums, partials);
        if (pl.n_heavy > 0)
            hipLaunchKernelGGL(gat_source_sums_finish_kernel, dim3(heavy_grid(pl.n_heavy)), dim3(kBlockThreads), 0, s, pl, node_sums, partials);
    }
    return check_launch(what);
}

int ihg_gat_symmetrize(const float* ds, const int32_t* mirror, int64_t nnz, float* ds_sym, ihg_stream_t stream) {
    if (nnz < 0) return fail(IHG_ERR_INVALID, "ihg_gat_symmetrize: bad size");
    if (nnz == 0) return IHG_OK;
    if (const int rc = check_pointers("ihg_gat_symmetrize", {ds, mirror, ds_sym}); rc != IHG_OK) return rc;
    hipLaunchKernelGGL(gat_symmetrize_kernel, dim3(flat_grid(nnz)), dim3(kBlockThreads), 0, static_cast<hipStream_t>(stream), ds, mirror, nnz, ds_sym);
    return check_launch("ihg_gat_symmetrize");
}

int ihg_gat_finish_bwd(const float* h, int64_t ld_h, const float* b, int64_t ld_b, const float* node_sums, const float* weight, int32_t head, int64_t n_rows,
                       int32_t dim, float* dh, int64_t ld_dh, float* dweight, float* dbias, void* workspace, int64_t workspace_bytes, ihg_stream_t stream) {
    const char* const what = "ihg_gat_finish_bwd";
    const bool product = head == IHG_GAT_PRODUCT;
    if (n_rows < 0 || dim <= 0 || ld_h < dim || ld_dh < dim || (product && ld_b < dim))
        return fail(IHG_ERR_INVALID, "%s: bad size (rows=%lld dim=%d)", what, (long long)n_rows, dim);
    if (const int rc = check_head(what, head); rc != IHG_OK) return rc;
    if (const int rc = check_pointers(what, {dweight, dbias, weight, workspace}); rc != IHG_OK) return rc;
    if (const int rc = check_workspace(what, workspace_bytes, ihg_gat_workspace_bytes(n_rows, 0, dim, head)); rc != IHG_OK) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (n_rows == 0) {
        launch_zero_floats(dweight, product ? dim : 2 * dim, s);
        launch_zero_floats(dbias, 1, s);
        return check_launch(what);
    }
    if (const int rc = check_pointers(what, {h, node_sums, dh}); rc != IHG_OK) return rc;
    if (product && b == nullptr) return fail(IHG_ERR_INVALID, "%s: null pointer", what);
    float* partials = static_cast<float*>(workspace);
    const int n_cols = (product ? dim : 2 * dim) + 1;
    const int64_t blocks = param_blocks(n_rows);
    hipLaunchKernelGGL(gat_param_partials_kernel, dim3(static_cast<unsigned>(blocks)), dim3(kBlockThreads), 0, s, h, ld_h, b, ld_b, node_sums, head, n_rows, dim, n_cols,
                       partials);
    hipLaunchKernelGGL(gat_param_finish_kernel, dim3((n_cols + kBlockThreads - 1) / kBlockThreads), dim3(kBlockThreads), 0, s, partials, blocks, n_cols,
                       product ? 0.5f : 1.f, dweight, dbias);
    launch_node_grad<true, true>(rows16(dim, ld_dh, dh) && aligned16(weight) && (!product || rows16(dim, ld_b, b)), dh, ld_dh, b, ld_b, node_sums, weight, head, n_rows,
                                 dim, s);
    return check_launch(what);
}

}  // extern "C"
