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
#include "attention.hpp"

namespace {

// ------------------------------------------------------------------------------------------------
// concat head: s[v] = (h[v] . w_src, h[v] . w_dst) once per node (GnnLayers.py:104, 111: w . [h_u | h_v] splits into two node terms)
// ------------------------------------------------------------------------------------------------
template <int VEC, int G>
__global__ __launch_bounds__(kBlockThreads) void gat_project_kernel(const float* __restrict__ h, int64_t ld_h, const float* __restrict__ w, int dim, int dim_vec,
                                                                    int64_t n_rows, float* __restrict__ s) {
    constexpr int GPW = kWave / G;
    const int lane = threadIdx.x & (kWave - 1);
    const int lig = lane & (G - 1);
    const int grp = lane / G;
    for (int64_t r0 = global_wave_id() * GPW; r0 < n_rows; r0 += global_wave_count() * GPW) {
        const int64_t r = r0 + grp;
        float a = 0.f, b = 0.f;
        if (r < n_rows) {
            for (int c = lig; c < dim_vec; c += G) {
                const Frag<VEC> x = Frag<VEC>::load(h + r * ld_h + c * VEC);
                a += frag_dot(x, Frag<VEC>::load(w + c * VEC));
                b += frag_dot(x, Frag<VEC>::load(w + dim + c * VEC));
            }
        }
        a = group_sum<G>(a);
        b = group_sum<G>(b);
        if (r < n_rows && lig == 0) {
            s[2 * r] = a;
            s[2 * r + 1] = b;
        }
    }
}

// ------------------------------------------------------------------------------------------------
// Softmax over every row (DGL edge_softmax, normalised per destination: GnnLayers.py:112).  Light rows are finished here; a segment of a split
// row leaves its (max, sum of exp(z - max)) in partials[2 seg ..].  CONCAT: z[p] = act(s_src[u] + s_dst[v] + c) is formed (and stored) here.
// ------------------------------------------------------------------------------------------------
template <bool CONCAT>
__global__ __launch_bounds__(kBlockThreads) void gat_softmax_kernel(const float* __restrict__ s, const float* __restrict__ bias, int act, Plan pl,
                                                                    float* __restrict__ z, float* __restrict__ alpha, float* __restrict__ alpha_mirror,
                                                                    float* __restrict__ partials) {
    constexpr int G = kScalarLanes, GPW = kWave / G;
    const int lane = threadIdx.x & (kWave - 1);
    const int lig = lane & (G - 1);
    const int grp = lane / G;
    const int64_t n_units = pl.n_segments + pl.n_rows;
    for (int64_t u0 = global_wave_id() * GPW; u0 < n_units; u0 += global_wave_count() * GPW) {
        const Unit un = unit_at(pl, u0 + grp);
        float m = -__builtin_huge_valf();
        if (CONCAT) {
            const float dst = un.len > 0 ? s[2 * un.row + 1] + bias[0] : 0.f;
            for (int i = lig; i < un.len; i += G) {
                const int p = un.begin + i;
                const float v = gat_act(s[2 * static_cast<int64_t>(pl.ids[p])] + dst, act);
                z[p] = v;
                m = fmaxf(m, v);
            }
        } else {
            for (int i = lig; i < un.len; i += G) m = fmaxf(m, z[un.begin + i]);
        }
        m = group_max<G>(m);
        float l = 0.f;
        for (int i = lig; i < un.len; i += G) l += expf(z[un.begin + i] - m);
        l = group_sum<G>(l);
        if (un.seg >= 0) {
            if (lig == 0) {
                partials[2 * un.seg] = m;
                partials[2 * un.seg + 1] = l;
            }
        } else if (un.row >= 0) {
            for (int i = lig; i < un.len; i += G) {
                const int p = un.begin + i;
                const float al = expf(z[p] - m) / l;
                alpha[p] = al;
                alpha_mirror[pl.mirror[p]] = al;
            }
        }
    }
}

// One workgroup per split row: merge its segments' (max, sum) in a fixed tree, then write alpha over the row's entries.
__global__ __launch_bounds__(kBlockThreads) void gat_softmax_finish_kernel(Plan pl, const float* __restrict__ z, const float* __restrict__ partials,
                                                                           float* __restrict__ alpha, float* __restrict__ alpha_mirror) {
    __shared__ float rm[kBlockThreads], rl[kBlockThreads];
    const int t = threadIdx.x;
    for (int64_t hr = blockIdx.x; hr < pl.n_heavy; hr += gridDim.x) {
        const int s0 = pl.heavy_segptr[hr], s1 = pl.heavy_segptr[hr + 1];
        float m = -__builtin_huge_valf(), l = 0.f;
        for (int sg = s0 + t; sg < s1; sg += kBlockThreads) merge_max_sum(m, l, partials[2 * static_cast<int64_t>(sg)], partials[2 * static_cast<int64_t>(sg) + 1]);
        rm[t] = m;
        rl[t] = l;
        __syncthreads();
        for (int o = kBlockThreads / 2; o > 0; o >>= 1) {
            if (t < o) {
                float mm = rm[t], ll = rl[t];
                merge_max_sum(mm, ll, rm[t + o], rl[t + o]);
                rm[t] = mm;
                rl[t] = ll;
            }
            __syncthreads();
        }
        const float mx = rm[0], den = rl[0];
        __syncthreads();
        const int64_t row = pl.heavy_rows[hr];
        for (int p = pl.rowptr[row] + t; p < pl.rowptr[row + 1]; p += kBlockThreads) {
            const float al = expf(z[p] - mx) / den;
            alpha[p] = al;
            alpha_mirror[pl.mirror[p]] = al;
        }
    }
}

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

// dh[v] += node_sums[2 v] w_src + node_sums[2 v + 1] w_dst (concat)   |   dh[v] += w * b[v] (product)
template <int VEC>
__global__ __launch_bounds__(kBlockThreads) void gat_combine_kernel(float* __restrict__ dh, int64_t ld_dh, const float* __restrict__ b, int64_t ld_b,
                                                                    const float* __restrict__ node_sums, const float* __restrict__ w, int head, int64_t n_rows,
                                                                    int dim, int dim_vec) {
    const int64_t total = n_rows * dim_vec;
    for (int64_t i = static_cast<int64_t>(blockIdx.x) * kBlockThreads + threadIdx.x; i < total; i += static_cast<int64_t>(gridDim.x) * kBlockThreads) {
        const int64_t r = i / dim_vec;
        const int c = static_cast<int>(i - r * dim_vec);
        Frag<VEC> acc = Frag<VEC>::load(dh + r * ld_dh + c * VEC);
        if (head == IHG_GAT_CONCAT) {
            Frag<VEC> t = Frag<VEC>::zero();
            t.add_scaled(Frag<VEC>::load(w + c * VEC), node_sums[2 * r]);
            t.add_scaled(Frag<VEC>::load(w + dim + c * VEC), node_sums[2 * r + 1]);
            acc.add(t);
        } else {
            acc.add(frag_mul(Frag<VEC>::load(w + c * VEC), Frag<VEC>::load(b + r * ld_b + c * VEC)));
        }
        acc.store(dh + r * ld_dh + c * VEC);
    }
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

template <int VEC>
void launch_project(const float* h, int64_t ld_h, const float* w, int dim, int64_t n_rows, float* s, hipStream_t st) {
    const int dim_vec = dim / VEC;
#define IHG_GAT_PROJ(G) \
    hipLaunchKernelGGL((gat_project_kernel<VEC, G>), dim3(gat_grid((n_rows + kWave / G - 1) / (kWave / G))), dim3(kBlockThreads), 0, st, h, ld_h, w, dim, dim_vec, n_rows, s)
    switch (gat_group_lanes(dim_vec)) {
        case 4: IHG_GAT_PROJ(4); break;
        case 8: IHG_GAT_PROJ(8); break;
        case 16: IHG_GAT_PROJ(16); break;
        case 32: IHG_GAT_PROJ(32); break;
        default: IHG_GAT_PROJ(64); break;
    }
#undef IHG_GAT_PROJ
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
    const Plan pl = make_plan(rowptr, ids, mirror, row_order, n_rows, heavy_threshold, seg_begin, seg_end, seg_row, n_segments, heavy_rows, heavy_segptr, n_heavy);
    const int rc = check_plan("ihg_gat_attention_fwd", pl, head, activation, dim);
    if (rc != IHG_OK) return rc;
    if (ld_h < dim) return fail(IHG_ERR_INVALID, "ihg_gat_attention_fwd: ld_h %lld < dim %d", (long long)ld_h, dim);
    if (n_rows == 0) return IHG_OK;
    if (h == nullptr || weight == nullptr || bias == nullptr || z == nullptr || alpha == nullptr || alpha_mirror == nullptr || workspace == nullptr)
        return fail(IHG_ERR_INVALID, "ihg_gat_attention_fwd: null pointer");
    const int64_t need = ihg_gat_workspace_bytes(n_rows, pl.n_segments, dim, head);
    if (workspace_bytes < need) return fail(IHG_ERR_WORKSPACE, "ihg_gat_attention_fwd: workspace %lld < %lld bytes", (long long)workspace_bytes, (long long)need);
    hipStream_t s = static_cast<hipStream_t>(stream);
    float* ws = static_cast<float*>(workspace);
    float* proj = ws;                                                    // concat: [n_rows, 2]
    float* partials = ws + (head == IHG_GAT_CONCAT ? 2 * n_rows : 0);    // [n_segments, 2]
    const int grid = gat_grid((pl.n_segments + n_rows + kWave / kScalarLanes - 1) / (kWave / kScalarLanes));
    if (head == IHG_GAT_CONCAT) {
        if (vec4_ok(dim, ld_h, h, 0, nullptr, weight)) launch_project<4>(h, ld_h, weight, dim, n_rows, proj, s);
        else launch_project<1>(h, ld_h, weight, dim, n_rows, proj, s);
        hipLaunchKernelGGL((gat_softmax_kernel<true>), dim3(grid), dim3(kBlockThreads), 0, s, proj, bias, activation, pl, z, alpha, alpha_mirror, partials);
    } else {
        if (vec4_ok(dim, ld_h, h, 0, nullptr, weight)) launch_row_dot<4>(h, ld_h, weight, h, ld_h, bias, activation, pl, dim, z, s);
        else launch_row_dot<1>(h, ld_h, weight, h, ld_h, bias, activation, pl, dim, z, s);
        hipLaunchKernelGGL((gat_softmax_kernel<false>), dim3(grid), dim3(kBlockThreads), 0, s, nullptr, bias, activation, pl, z, alpha, alpha_mirror, partials);
    }
    if (pl.n_heavy > 0)
        hipLaunchKernelGGL(gat_softmax_finish_kernel, dim3(heavy_grid(pl.n_heavy)), dim3(kBlockThreads), 0, s, pl, z, partials, alpha, alpha_mirror);
    return check_launch("ihg_gat_attention_fwd");
}

int ihg_gat_scores_bwd(const float* h, int64_t ld_h, const float* dout, int64_t ld_dout, const int32_t* rowptr, const int32_t* ids, const int32_t* mirror,
                       const int32_t* row_order, int64_t n_rows, int32_t dim, int32_t head, int32_t activation, int32_t heavy_threshold, const int32_t* seg_begin,
                       const int32_t* seg_end, const int32_t* seg_row, int64_t n_segments, const int32_t* heavy_rows, const int32_t* heavy_segptr, int64_t n_heavy,
                       const float* z, const float* alpha, float* ds, float* node_sums, void* workspace, int64_t workspace_bytes, ihg_stream_t stream) {
    const Plan pl = make_plan(rowptr, ids, mirror, row_order, n_rows, heavy_threshold, seg_begin, seg_end, seg_row, n_segments, heavy_rows, heavy_segptr, n_heavy);
    const int rc = check_plan("ihg_gat_scores_bwd", pl, head, activation, dim);
    if (rc != IHG_OK) return rc;
    if (ld_h < dim || ld_dout < dim) return fail(IHG_ERR_INVALID, "ihg_gat_scores_bwd: bad row stride");
    if (n_rows == 0) return IHG_OK;
    if (h == nullptr || dout == nullptr || z == nullptr || alpha == nullptr || ds == nullptr || node_sums == nullptr || workspace == nullptr)
        return fail(IHG_ERR_INVALID, "ihg_gat_scores_bwd: null pointer");
    const int64_t need = ihg_gat_workspace_bytes(n_rows, pl.n_segments, dim, head);
    if (workspace_bytes < need) return fail(IHG_ERR_WORKSPACE, "ihg_gat_scores_bwd: workspace %lld < %lld bytes", (long long)workspace_bytes, (long long)need);
    hipStream_t s = static_cast<hipStream_t>(stream);
    float* partials = static_cast<float*>(workspace);                     // [n_segments]
    // d alpha[p] = dout[v] . h[u]   (u_mul_e_sum's gradient with respect to the edge weight, GnnLayers.py:114)
    const bool wide = dim % 4 == 0 && ld_h % 4 == 0 && ld_dout % 4 == 0 && aligned16(h) && aligned16(dout);
    if (wide) launch_row_dot<4>(dout, ld_dout, nullptr, h, ld_h, nullptr, -1, pl, dim, ds, s);
    else launch_row_dot<1>(dout, ld_dout, nullptr, h, ld_h, nullptr, -1, pl, dim, ds, s);
    const int grid = gat_grid((pl.n_segments + n_rows + kWave / kScalarLanes - 1) / (kWave / kScalarLanes));
    hipLaunchKernelGGL(gat_softmax_bwd_kernel, dim3(grid), dim3(kBlockThreads), 0, s, z, alpha, ds, activation, pl, node_sums, partials);
    if (pl.n_heavy > 0)
        hipLaunchKernelGGL(gat_softmax_bwd_finish_kernel, dim3(heavy_grid(pl.n_heavy)), dim3(kBlockThreads), 0, s, z, alpha, ds, activation, pl, node_sums, partials);
    if (head == IHG_GAT_CONCAT) {
        hipLaunchKernelGGL(gat_source_sums_kernel, dim3(grid), dim3(kBlockThreads), 0, s, ds, pl, node_sums, partials);
        if (pl.n_heavy > 0)
            hipLaunchKernelGGL(gat_source_sums_finish_kernel, dim3(heavy_grid(pl.n_heavy)), dim3(kBlockThreads), 0, s, pl, node_sums, partials);
    }
    return check_launch("ihg_gat_scores_bwd");
}

int ihg_gat_symmetrize(const float* ds, const int32_t* mirror, int64_t nnz, float* ds_sym, ihg_stream_t stream) {
    if (nnz < 0) return fail(IHG_ERR_INVALID, "ihg_gat_symmetrize: bad size");
    if (nnz == 0) return IHG_OK;
    if (ds == nullptr || mirror == nullptr || ds_sym == nullptr) return fail(IHG_ERR_INVALID, "ihg_gat_symmetrize: null pointer");
    hipLaunchKernelGGL(gat_symmetrize_kernel, dim3(flat_grid(nnz)), dim3(kBlockThreads), 0, static_cast<hipStream_t>(stream), ds, mirror, nnz, ds_sym);
    return check_launch("ihg_gat_symmetrize");
}

int ihg_gat_finish_bwd(const float* h, int64_t ld_h, const float* b, int64_t ld_b, const float* node_sums, const float* weight, int32_t head, int64_t n_rows,
                       int32_t dim, float* dh, int64_t ld_dh, float* dweight, float* dbias, void* workspace, int64_t workspace_bytes, ihg_stream_t stream) {
    if (n_rows < 0 || dim <= 0 || ld_h < dim || ld_dh < dim || (head == IHG_GAT_PRODUCT && ld_b < dim))
        return fail(IHG_ERR_INVALID, "ihg_gat_finish_bwd: bad size (rows=%lld dim=%d)", (long long)n_rows, dim);
    if (head != IHG_GAT_CONCAT && head != IHG_GAT_PRODUCT) return fail(IHG_ERR_INVALID, "ihg_gat_finish_bwd: unknown head %d", head);
    if (dweight == nullptr || dbias == nullptr || weight == nullptr || workspace == nullptr) return fail(IHG_ERR_INVALID, "ihg_gat_finish_bwd: null pointer");
    const int64_t need = ihg_gat_workspace_bytes(n_rows, 0, dim, head);
    if (workspace_bytes < need) return fail(IHG_ERR_WORKSPACE, "ihg_gat_finish_bwd: workspace %lld < %lld bytes", (long long)workspace_bytes, (long long)need);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int n_cols = (head == IHG_GAT_CONCAT ? 2 * dim : dim) + 1;
    if (n_rows == 0) {
        launch_zero_floats(dweight, n_cols - 1, s);
        launch_zero_floats(dbias, 1, s);
        return check_launch("ihg_gat_finish_bwd");
    }
    if (h == nullptr || node_sums == nullptr || dh == nullptr || (head == IHG_GAT_PRODUCT && b == nullptr)) return fail(IHG_ERR_INVALID, "ihg_gat_finish_bwd: null pointer");
    float* partials = static_cast<float*>(workspace);
    const int64_t blocks = param_blocks(n_rows);
    hipLaunchKernelGGL(gat_param_partials_kernel, dim3(static_cast<unsigned>(blocks)), dim3(kBlockThreads), 0, s, h, ld_h, b, ld_b, node_sums, head, n_rows, dim, n_cols,
                       partials);
    hipLaunchKernelGGL(gat_param_finish_kernel, dim3((n_cols + kBlockThreads - 1) / kBlockThreads), dim3(kBlockThreads), 0, s, partials, blocks, n_cols,
                       head == IHG_GAT_PRODUCT ? 0.5f : 1.f, dweight, dbias);
    const bool product = head == IHG_GAT_PRODUCT;
    if (vec4_ok(dim, ld_dh, dh, product ? ld_b : 0, product ? b : nullptr, weight))
        hipLaunchKernelGGL((gat_combine_kernel<4>), dim3(flat_grid(n_rows * (dim / 4))), dim3(kBlockThreads), 0, s, dh, ld_dh, b, ld_b, node_sums, weight, head, n_rows,
                           dim, dim / 4);
    else
        hipLaunchKernelGGL((gat_combine_kernel<1>), dim3(flat_grid(n_rows * dim)), dim3(kBlockThreads), 0, s, dh, ld_dh, b, ld_b, node_sums, weight, head, n_rows, dim, dim);
    return check_launch("ihg_gat_finish_bwd");
}

}  // extern "C"
