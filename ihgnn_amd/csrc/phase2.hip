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
#include "attention.hpp"

namespace {

// out[r] = x[r] . w
template <int VEC, int G>
__global__ __launch_bounds__(kBlockThreads) void p2_project_kernel(const float* __restrict__ x, int64_t ld_x, const float* __restrict__ w, int dim_vec, int64_t n_rows,
                                                                   float* __restrict__ out) {
    constexpr int GPW = kWave / G;
    const int lane = threadIdx.x & (kWave - 1);
    const int lig = lane & (G - 1);
    const int grp = lane / G;
    for (int64_t r0 = global_wave_id() * GPW; r0 < n_rows; r0 += global_wave_count() * GPW) {
        const int64_t r = r0 + grp;
        float a = 0.f;
        if (r < n_rows)
            for (int c = lig; c < dim_vec; c += G) a += frag_dot(Frag<VEC>::load(x + r * ld_x + c * VEC), Frag<VEC>::load(w + c * VEC));
        a = group_sum<G>(a);
        if (r < n_rows && lig == 0) out[r] = a;
    }
}

__device__ __forceinline__ float mult_of(const float* __restrict__ mult, int e) { return mult != nullptr ? mult[e] : 1.f; }

// Softmax over every node row.  Light rows are finished here; a segment of a split row leaves its (max, sum of m exp(z - max)) in partials[2 seg ..].
// CONCAT: z[p] = act(a[e] + b[v] + c) is formed (and stored) here.
template <bool CONCAT>
__global__ __launch_bounds__(kBlockThreads) void p2_softmax_kernel(const float* __restrict__ a, const float* __restrict__ b, const float* __restrict__ bias,
                                                                   const float* __restrict__ mult, int act, Plan pl, float* __restrict__ z, float* __restrict__ alpha,
                                                                   float* __restrict__ alpha_edge, float* __restrict__ partials) {
    constexpr int G = kScalarLanes, GPW = kWave / G;
    const int lane = threadIdx.x & (kWave - 1);
    const int lig = lane & (G - 1);
    const int grp = lane / G;
    const int64_t n_units = pl.n_segments + pl.n_rows;
    for (int64_t u0 = global_wave_id() * GPW; u0 < n_units; u0 += global_wave_count() * GPW) {
        const Unit un = unit_at(pl, u0 + grp);
        float m = -__builtin_huge_valf();
        if (CONCAT) {
            const float dst = un.len > 0 ? b[un.row] + bias[0] : 0.f;
            for (int i = lig; i < un.len; i += G) {
                const int p = un.begin + i;
                const float v = gat_act(a[pl.ids[p]] + dst, act);
                z[p] = v;
                m = fmaxf(m, v);
            }
        } else {
            for (int i = lig; i < un.len; i += G) m = fmaxf(m, z[un.begin + i]);
        }
        m = group_max<G>(m);
        float l = 0.f;
        for (int i = lig; i < un.len; i += G) l += mult_of(mult, pl.ids[un.begin + i]) * expf(z[un.begin + i] - m);
        l = group_sum<G>(l);
        if (un.seg >= 0) {
            if (lig == 0) {
                partials[2 * un.seg] = m;
                partials[2 * un.seg + 1] = l;
            }
        } else if (un.row >= 0) {
            for (int i = lig; i < un.len; i += G) {
                const int p = un.begin + i;
                const float al = mult_of(mult, pl.ids[p]) * expf(z[p] - m) / l;
                alpha[p] = al;
                alpha_edge[pl.mirror[p]] = al;
            }
        }
    }
}

// One workgroup per split row: merge its segments' (max, sum) in a fixed tree, then write alpha over the row's entries.
__global__ __launch_bounds__(kBlockThreads) void p2_softmax_finish_kernel(Plan pl, const float* __restrict__ z, const float* __restrict__ mult,
                                                                          const float* __restrict__ partials, float* __restrict__ alpha,
                                                                          float* __restrict__ alpha_edge) {
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
            const float al = mult_of(mult, pl.ids[p]) * expf(z[p] - mx) / den;
            alpha[p] = al;
            alpha_edge[pl.mirror[p]] = al;
        }
    }
}

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

// dh[v] = node_sums[2 v + 1] w_dst (concat)   |   dh[v] = w * b[v] (product)
template <int VEC>
__global__ __launch_bounds__(kBlockThreads) void p2_node_grad_kernel(float* __restrict__ dh, int64_t ld_dh, const float* __restrict__ b, int64_t ld_b,
                                                                     const float* __restrict__ node_sums, const float* __restrict__ w, int head, int64_t n_rows,
                                                                     int dim, int dim_vec) {
    const int64_t total = n_rows * dim_vec;
    for (int64_t i = static_cast<int64_t>(blockIdx.x) * kBlockThreads + threadIdx.x; i < total; i += static_cast<int64_t>(gridDim.x) * kBlockThreads) {
        const int64_t r = i / dim_vec;
        const int c = static_cast<int>(i - r * dim_vec);
        Frag<VEC> acc = Frag<VEC>::zero();
        if (head == IHG_GAT_CONCAT) acc.add_scaled(Frag<VEC>::load(w + dim + c * VEC), node_sums[2 * r + 1]);
        else acc = frag_mul(Frag<VEC>::load(w + c * VEC), Frag<VEC>::load(b + r * ld_b + c * VEC));
        acc.store(dh + r * ld_dh + c * VEC);
    }
}

// Column sums over the rows of a table, kParamRows rows per workgroup (then the workgroups' partials in a fixed tree, p2_colsum_finish_kernel):
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

template <int VEC>
void launch_p2_project(const float* x, int64_t ld_x, const float* w, int dim, int64_t n_rows, float* out, hipStream_t st) {
    const int dim_vec = dim / VEC;
#define IHG_P2_PROJ(G) \
    hipLaunchKernelGGL((p2_project_kernel<VEC, G>), dim3(gat_grid((n_rows + kWave / G - 1) / (kWave / G))), dim3(kBlockThreads), 0, st, x, ld_x, w, dim_vec, n_rows, out)
    switch (gat_group_lanes(dim_vec)) {
        case 4: IHG_P2_PROJ(4); break;
        case 8: IHG_P2_PROJ(8); break;
        case 16: IHG_P2_PROJ(16); break;
        case 32: IHG_P2_PROJ(32); break;
        default: IHG_P2_PROJ(64); break;
    }
#undef IHG_P2_PROJ
}

template <int VEC, bool PRODUCT>
void launch_p2_edges_bwd(const float* dout, int64_t ld_dout, const float* h, int64_t ld_h, const int32_t* i3, const float* alpha_edge, const float* ds_edge,
                         const float* w, int64_t n_edges, int dim, float* def, int64_t ld_def, hipStream_t st) {
    const int dim_vec = dim / VEC;
#define IHG_P2_EDGE(G)                                                                                                                                      \
    hipLaunchKernelGGL((p2_edges_bwd_kernel<VEC, G, PRODUCT>), dim3(gat_grid((n_edges + kWave / G - 1) / (kWave / G))), dim3(kBlockThreads), 0, st, dout, ld_dout, h, \
                       ld_h, i3, alpha_edge, ds_edge, w, n_edges, dim_vec, def, ld_def)
    switch (gat_group_lanes(dim_vec)) {
        case 4: IHG_P2_EDGE(4); break;
        case 8: IHG_P2_EDGE(8); break;
        case 16: IHG_P2_EDGE(16); break;
        case 32: IHG_P2_EDGE(32); break;
        default: IHG_P2_EDGE(64); break;
    }
#undef IHG_P2_EDGE
}

// threads side by side on a row of the column sums: the smallest power of two >= n_cols, at most a workgroup
inline int colsum_width(int n_cols) {
    int cw = 4;
    while (cw < n_cols && cw < kBlockThreads) cw <<= 1;
    return cw;
}

bool rows16(int32_t dim, int64_t ld, const void* p) { return dim % 4 == 0 && ld % 4 == 0 && aligned16(p); }

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
    const Plan pl = make_plan(rowptr, ids, pos, row_order, n_rows, heavy_threshold, seg_begin, seg_end, seg_row, n_segments, heavy_rows, heavy_segptr, n_heavy);
    const int rc = check_plan("ihg_phase2_attention_fwd", pl, head, activation, dim);
    if (rc != IHG_OK) return rc;
    if (n_edges < 0 || ld_h < dim || ld_ef < dim) return fail(IHG_ERR_INVALID, "ihg_phase2_attention_fwd: bad size or row stride");
    if (n_rows == 0 || n_edges == 0) return IHG_OK;
    if (h == nullptr || ef == nullptr || weight == nullptr || bias == nullptr || z == nullptr || alpha == nullptr || alpha_edge == nullptr || workspace == nullptr)
        return fail(IHG_ERR_INVALID, "ihg_phase2_attention_fwd: null pointer");
    const int64_t need = ihg_phase2_workspace_bytes(n_rows, n_edges, pl.n_segments, dim, head);
    if (workspace_bytes < need) return fail(IHG_ERR_WORKSPACE, "ihg_phase2_attention_fwd: workspace %lld < %lld bytes", (long long)workspace_bytes, (long long)need);
    hipStream_t s = static_cast<hipStream_t>(stream);
    float* ws = static_cast<float*>(workspace);
    const bool concat = head == IHG_GAT_CONCAT;
    float* a = ws;                                                   // concat: [n_edges]
    float* b = ws + (concat ? n_edges : 0);                          // concat: [n_rows]
    float* partials = b + (concat ? n_rows : 0);                     // [n_segments, 2]
    const int grid = gat_grid((pl.n_segments + n_rows + kWave / kScalarLanes - 1) / (kWave / kScalarLanes));
    if (concat) {
        if (rows16(dim, ld_ef, ef) && aligned16(weight)) launch_p2_project<4>(ef, ld_ef, weight, dim, n_edges, a, s);
        else launch_p2_project<1>(ef, ld_ef, weight, dim, n_edges, a, s);
        if (rows16(dim, ld_h, h) && aligned16(weight)) launch_p2_project<4>(h, ld_h, weight + dim, dim, n_rows, b, s);
        else launch_p2_project<1>(h, ld_h, weight + dim, dim, n_rows, b, s);
        hipLaunchKernelGGL((p2_softmax_kernel<true>), dim3(grid), dim3(kBlockThreads), 0, s, a, b, bias, edge_weight, activation, pl, z, alpha, alpha_edge, partials);
    } else {
        // z[p] = act(w . (h[v] * ef[e]) + c)
        if (vec4_ok(dim, ld_h, h, ld_ef, ef, weight)) launch_row_dot<4>(h, ld_h, weight, ef, ld_ef, bias, activation, pl, dim, z, s);
        else launch_row_dot<1>(h, ld_h, weight, ef, ld_ef, bias, activation, pl, dim, z, s);
        hipLaunchKernelGGL((p2_softmax_kernel<false>), dim3(grid), dim3(kBlockThreads), 0, s, nullptr, nullptr, bias, edge_weight, activation, pl, z, alpha, alpha_edge,
                           partials);
    }
    if (pl.n_heavy > 0)
        hipLaunchKernelGGL(p2_softmax_finish_kernel, dim3(heavy_grid(pl.n_heavy)), dim3(kBlockThreads), 0, s, pl, z, edge_weight, partials, alpha, alpha_edge);
    return check_launch("ihg_phase2_attention_fwd");
}

int ihg_phase2_scores_bwd(const float* ef, int64_t ld_ef, const float* dout, int64_t ld_dout, const int32_t* rowptr, const int32_t* ids, const int32_t* pos,
                          const int32_t* row_order, int64_t n_rows, int64_t n_edges, int32_t dim, int32_t head, int32_t activation, int32_t heavy_threshold,
                          const int32_t* seg_begin, const int32_t* seg_end, const int32_t* seg_row, int64_t n_segments, const int32_t* heavy_rows,
                          const int32_t* heavy_segptr, int64_t n_heavy, const float* z, const float* alpha, float* ds, float* ds_edge, float* node_sums,
                          void* workspace, int64_t workspace_bytes, ihg_stream_t stream) {
    const Plan pl = make_plan(rowptr, ids, pos, row_order, n_rows, heavy_threshold, seg_begin, seg_end, seg_row, n_segments, heavy_rows, heavy_segptr, n_heavy);
    const int rc = check_plan("ihg_phase2_scores_bwd", pl, head, activation, dim);
    if (rc != IHG_OK) return rc;
    if (n_edges < 0 || ld_ef < dim || ld_dout < dim) return fail(IHG_ERR_INVALID, "ihg_phase2_scores_bwd: bad size or row stride");
    if (n_rows == 0 || n_edges == 0) return IHG_OK;
    if (ef == nullptr || dout == nullptr || z == nullptr || alpha == nullptr || ds == nullptr || ds_edge == nullptr || node_sums == nullptr || workspace == nullptr)
        return fail(IHG_ERR_INVALID, "ihg_phase2_scores_bwd: null pointer");
    const int64_t need = ihg_phase2_workspace_bytes(n_rows, n_edges, pl.n_segments, dim, head);
    if (workspace_bytes < need) return fail(IHG_ERR_WORKSPACE, "ihg_phase2_scores_bwd: workspace %lld < %lld bytes", (long long)workspace_bytes, (long long)need);
    hipStream_t s = static_cast<hipStream_t>(stream);
    float* partials = static_cast<float*>(workspace);                     // [n_segments]
    // d alpha[p] = dout[v] . ef[e]
    if (rows16(dim, ld_ef, ef) && rows16(dim, ld_dout, dout)) launch_row_dot<4>(dout, ld_dout, nullptr, ef, ld_ef, nullptr, -1, pl, dim, ds, s);
    else launch_row_dot<1>(dout, ld_dout, nullptr, ef, ld_ef, nullptr, -1, pl, dim, ds, s);
    const int grid = gat_grid((pl.n_segments + n_rows + kWave / kScalarLanes - 1) / (kWave / kScalarLanes));
    hipLaunchKernelGGL(gat_softmax_bwd_kernel, dim3(grid), dim3(kBlockThreads), 0, s, z, alpha, ds, activation, pl, node_sums, partials);
    if (pl.n_heavy > 0)
        hipLaunchKernelGGL(gat_softmax_bwd_finish_kernel, dim3(heavy_grid(pl.n_heavy)), dim3(kBlockThreads), 0, s, z, alpha, ds, activation, pl, node_sums, partials);
    hipLaunchKernelGGL(p2_to_edge_slots_kernel, dim3(flat_grid(3 * n_edges)), dim3(kBlockThreads), 0, s, ds, pos, 3 * n_edges, ds_edge);
    return check_launch("ihg_phase2_scores_bwd");
}

int ihg_phase2_edges_bwd(const float* dout, int64_t ld_dout, const float* h, int64_t ld_h, const int32_t* i3, const float* alpha_edge, const float* ds_edge,
                         const float* weight, int32_t head, int64_t n_edges, int32_t dim, float* def, int64_t ld_def, ihg_stream_t stream) {
    if (n_edges < 0 || dim <= 0 || ld_dout < dim || ld_h < dim || ld_def < dim) return fail(IHG_ERR_INVALID, "ihg_phase2_edges_bwd: bad size (edges=%lld dim=%d)", (long long)n_edges, dim);
    if (head != IHG_GAT_CONCAT && head != IHG_GAT_PRODUCT) return fail(IHG_ERR_INVALID, "ihg_phase2_edges_bwd: unknown head %d", head);
    if (n_edges == 0) return IHG_OK;
    if (dout == nullptr || h == nullptr || i3 == nullptr || alpha_edge == nullptr || ds_edge == nullptr || weight == nullptr || def == nullptr)
        return fail(IHG_ERR_INVALID, "ihg_phase2_edges_bwd: null pointer");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const bool wide = rows16(dim, ld_dout, dout) && rows16(dim, ld_h, h) && rows16(dim, ld_def, def) && aligned16(weight);
    if (head == IHG_GAT_PRODUCT) {
        if (wide) launch_p2_edges_bwd<4, true>(dout, ld_dout, h, ld_h, i3, alpha_edge, ds_edge, weight, n_edges, dim, def, ld_def, s);
        else launch_p2_edges_bwd<1, true>(dout, ld_dout, h, ld_h, i3, alpha_edge, ds_edge, weight, n_edges, dim, def, ld_def, s);
    } else {
        if (wide) launch_p2_edges_bwd<4, false>(dout, ld_dout, h, ld_h, i3, alpha_edge, ds_edge, weight, n_edges, dim, def, ld_def, s);
        else launch_p2_edges_bwd<1, false>(dout, ld_dout, h, ld_h, i3, alpha_edge, ds_edge, weight, n_edges, dim, def, ld_def, s);
    }
    return check_launch("ihg_phase2_edges_bwd");
}

int ihg_phase2_finish_bwd(const float* h, int64_t ld_h, const float* ef, int64_t ld_ef, const float* b, int64_t ld_b, const float* node_sums, const float* ds_edge,
                          const float* weight, int32_t head, int64_t n_rows, int64_t n_edges, int32_t dim, float* dh, int64_t ld_dh, float* dweight, float* dbias,
                          void* workspace, int64_t workspace_bytes, ihg_stream_t stream) {
    if (n_rows < 0 || n_edges < 0 || dim <= 0 || ld_h < dim || ld_dh < dim || (head == IHG_GAT_PRODUCT && ld_b < dim) || (head == IHG_GAT_CONCAT && ld_ef < dim))
        return fail(IHG_ERR_INVALID, "ihg_phase2_finish_bwd: bad size (rows=%lld edges=%lld dim=%d)", (long long)n_rows, (long long)n_edges, dim);
    if (head != IHG_GAT_CONCAT && head != IHG_GAT_PRODUCT) return fail(IHG_ERR_INVALID, "ihg_phase2_finish_bwd: unknown head %d", head);
    if (dweight == nullptr || dbias == nullptr || weight == nullptr || workspace == nullptr) return fail(IHG_ERR_INVALID, "ihg_phase2_finish_bwd: null pointer");
    const int64_t need = ihg_phase2_workspace_bytes(n_rows, n_edges, 0, dim, head);
    if (workspace_bytes < need) return fail(IHG_ERR_WORKSPACE, "ihg_phase2_finish_bwd: workspace %lld < %lld bytes", (long long)workspace_bytes, (long long)need);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const bool concat = head == IHG_GAT_CONCAT;
    if (n_rows == 0 || n_edges == 0) {
        launch_zero_floats(dweight, concat ? 2 * dim : dim, s);
        launch_zero_floats(dbias, 1, s);
        return check_launch("ihg_phase2_finish_bwd");
    }
    if (h == nullptr || node_sums == nullptr || dh == nullptr || (concat ? (ef == nullptr || ds_edge == nullptr) : b == nullptr))
        return fail(IHG_ERR_INVALID, "ihg_phase2_finish_bwd: null pointer");
    float* node_partials = static_cast<float*>(workspace);
    const int64_t node_blocks = param_blocks(n_rows);
    float* edge_partials = node_partials + node_blocks * (dim + 1);
    if (concat) {
        // dw_src = sum_e (sum_k ds_edge[e, k]) ef[e]   |   dw_dst = sum_v S[v] h[v],  dc = sum_v S[v]
        const int64_t edge_blocks = param_blocks(n_edges);
        hipLaunchKernelGGL(p2_colsum_partials_kernel<3>, dim3(static_cast<unsigned>(edge_blocks)), dim3(kBlockThreads), 0, s, ef, ld_ef, nullptr, 0, ds_edge, 3, n_edges, dim,
                           dim, colsum_width(dim), edge_partials);
        hipLaunchKernelGGL(p2_colsum_finish_kernel, dim3(dim), dim3(kBlockThreads), 0, s, edge_partials, edge_blocks, dim, dim, dweight, dbias);
        hipLaunchKernelGGL(p2_colsum_partials_kernel<1>, dim3(static_cast<unsigned>(node_blocks)), dim3(kBlockThreads), 0, s, h, ld_h, nullptr, 0, node_sums + 1, 2, n_rows, dim,
                           dim + 1, colsum_width(dim), node_partials);
        hipLaunchKernelGGL(p2_colsum_finish_kernel, dim3(dim + 1), dim3(kBlockThreads), 0, s, node_partials, node_blocks, dim + 1, dim, dweight + dim, dbias);
    } else {
        // dw = sum_v h[v] * b[v]   (b = K7(ef, entry_scale = ds)),  dc = sum_v S[v]
        hipLaunchKernelGGL(p2_colsum_partials_kernel<1>, dim3(static_cast<unsigned>(node_blocks)), dim3(kBlockThreads), 0, s, h, ld_h, b, ld_b, node_sums + 1, 2, n_rows, dim,
                           dim + 1, colsum_width(dim), node_partials);
        hipLaunchKernelGGL(p2_colsum_finish_kernel, dim3(dim + 1), dim3(kBlockThreads), 0, s, node_partials, node_blocks, dim + 1, dim, dweight, dbias);
    }
    const bool wide = rows16(dim, ld_dh, dh) && aligned16(weight) && (concat || rows16(dim, ld_b, b));
    if (wide)
        hipLaunchKernelGGL((p2_node_grad_kernel<4>), dim3(flat_grid(n_rows * (dim / 4))), dim3(kBlockThreads), 0, s, dh, ld_dh, b, ld_b, node_sums, weight, head, n_rows, dim,
                           dim / 4);
    else
        hipLaunchKernelGGL((p2_node_grad_kernel<1>), dim3(flat_grid(n_rows * dim)), dim3(kBlockThreads), 0, s, dh, ld_dh, b, ld_b, node_sums, weight, head, n_rows, dim, dim);
    return check_launch("ihg_phase2_finish_bwd");
}

int ihg_phase2_add_rows(float* dst, int64_t ld_dst, const float* src, int64_t ld_src, int64_t n_rows, int32_t dim, ihg_stream_t stream) {
    if (n_rows < 0 || dim <= 0 || ld_dst < dim || ld_src < dim) return fail(IHG_ERR_INVALID, "ihg_phase2_add_rows: bad size (rows=%lld dim=%d)", (long long)n_rows, dim);
    if (n_rows == 0) return IHG_OK;
    if (dst == nullptr || src == nullptr) return fail(IHG_ERR_INVALID, "ihg_phase2_add_rows: null pointer");
    hipLaunchKernelGGL(p2_add_rows_kernel, dim3(flat_grid(n_rows * dim)), dim3(kBlockThreads), 0, static_cast<hipStream_t>(stream), dst, ld_dst, src, ld_src, n_rows, dim);
    return check_launch("ihg_phase2_add_rows");
}

}  // extern "C"
