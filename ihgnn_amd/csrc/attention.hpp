// attention.hpp - what the two attention translation units share (gat.hip: the GAT baseline over the pairwise graph; phase2.hip: the IHGNN layer's
// phase-2 attention over the node <- hyperedge incidence): activations, lane-group reductions, the row projection, the row gather-dot, the softmax forward and
// backward, the node-row gradient, and the launch and entry-point helpers.  The kernels walk K7's work list with its split rows (worklist.hpp).  A graph is a CSR
// whose row v lists the SOURCES of v's incoming edges; `mirror` maps entry p to its slot in the table that is walked from the other
// side (gat.hip: the reverse edge's position; phase2.hip: 3 e + type(v) of an edge-major [E, 3] table).  The kernels are __global__ templates with __restrict__
// on their own parameters (an inlined body behind a per-layer wrapper loses the qualifiers and with them the register allocation).
#pragma once
#include <initializer_list>

#include "common.hpp"
#include "worklist.hpp"

namespace {

constexpr int kScalarLanes = 16;          // lanes per work unit of the scalar passes (four units per wave)
constexpr int kParamRows = 512;           // node rows per workgroup of the parameter-gradient column sums

__device__ __forceinline__ float gat_act(float x, int act) {
    if (act == IHG_GAT_LEAKY_RELU) return x > 0.f ? x : 0.01f * x;           // nn.LeakyReLU() (slope 0.01)
    if (act == IHG_GAT_RELU) return x > 0.f ? x : 0.f;
    return tanhf(x);
}

// derivative from the OUTPUT, as torch takes it: leaky_relu_backward (x > 0 ? 1 : slope, so slope at 0), threshold_backward (y <= 0 -> 0), tanh_backward (1 - y^2)
__device__ __forceinline__ float gat_act_grad(float y, int act) {
    if (act == IHG_GAT_LEAKY_RELU) return y > 0.f ? 1.f : 0.01f;
    if (act == IHG_GAT_RELU) return y > 0.f ? 1.f : 0.f;
    return 1.f - y * y;
}

__device__ __forceinline__ float frag_dot(const Frag<4>& a, const Frag<4>& b) { return ((a.v.x * b.v.x + a.v.y * b.v.y) + a.v.z * b.v.z) + a.v.w * b.v.w; }
__device__ __forceinline__ float frag_dot(const Frag<1>& a, const Frag<1>& b) { return a.v * b.v; }
__device__ __forceinline__ Frag<4> frag_mul(const Frag<4>& a, const Frag<4>& b) { return {make_float4(a.v.x * b.v.x, a.v.y * b.v.y, a.v.z * b.v.z, a.v.w * b.v.w)}; }
__device__ __forceinline__ Frag<1> frag_mul(const Frag<1>& a, const Frag<1>& b) { return {a.v * b.v}; }

// butterfly over the G lanes of a group: every lane ends with the same bits (each step adds the same two values in either order)
template <int G>
__device__ __forceinline__ float group_sum(float v) {
#pragma unroll
    for (int o = G / 2; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
template <int G>
__device__ __forceinline__ float group_max(float v) {
#pragma unroll
    for (int o = G / 2; o >= 1; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}
// out[r, k] = x[r] . w[k dim ..] for the W = 1 or 2 weight vectors of the concatenation head, out [n_rows, W] (gat.hip: W = 2, both terms of a node from one
// load of its row; phase2.hip: W = 1 per table).  Two named sums, not an array over W: as an array the compiler packs the products another way and leaves the
// multiply-adds of a dot unfused - the same dot, rounded differently.
template <int VEC, int G, int W>
__global__ __launch_bounds__(kBlockThreads) void attn_project_kernel(const float* __restrict__ x, int64_t ld_x, const float* __restrict__ w, int dim, int dim_vec,
                                                                     int64_t n_rows, float* __restrict__ out) {
    static_assert(W == 1 || W == 2, "one or two weight vectors");
    constexpr int GPW = kWave / G;
    const int lane = threadIdx.x & (kWave - 1);
    const int lig = lane & (G - 1);
    const int grp = lane / G;
    for (int64_t r0 = global_wave_id() * GPW; r0 < n_rows; r0 += global_wave_count() * GPW) {
        const int64_t r = r0 + grp;
        float a = 0.f, b = 0.f;
        if (r < n_rows) {
            for (int c = lig; c < dim_vec; c += G) {
                const Frag<VEC> row = Frag<VEC>::load(x + r * ld_x + c * VEC);
                a += frag_dot(row, Frag<VEC>::load(w + c * VEC));
                if constexpr (W == 2) b += frag_dot(row, Frag<VEC>::load(w + dim + c * VEC));
            }
        }
        a = group_sum<G>(a);
        if constexpr (W == 2) b = group_sum<G>(b);
        if (r < n_rows && lig == 0) {
            out[W * r] = a;
            if constexpr (W == 2) out[W * r + 1] = b;
        }
    }
}

// ------------------------------------------------------------------------------------------------
// Row gather-dot: out[p] = act(bias + sum_k a[k] x[v][k] y[ids[p]][k]) for every entry p of row v (a NULL: ones; act < 0: neither activation nor bias).
//   product scores (GnnLayers.py:107, 111: x = y = h, a = w) and d alpha (x = dout, y = h).  G lanes per unit hold x[v] * a in registers,
//   eight neighbour rows in flight per lane, one butterfly per entry; lane j of the group keeps entry j of each chunk of G entries.
// ------------------------------------------------------------------------------------------------
template <int VEC, int G>
__global__ __launch_bounds__(kBlockThreads) void gat_row_dot_kernel(const float* __restrict__ x, int64_t ld_x, const float* __restrict__ a,
                                                                    const float* __restrict__ y, int64_t ld_y, const float* __restrict__ bias, int act,
                                                                    Plan pl, int dim_vec, float* __restrict__ out) {
    constexpr int GPW = kWave / G;
    constexpr int UNR = G < 8 ? G : 8;
    const int lane = threadIdx.x & (kWave - 1);
    const int lig = lane & (G - 1);
    const int grp = lane / G;
    const int group_base = lane & ~(G - 1);
    const int64_t n_units = pl.n_segments + pl.n_rows;
    const float c0 = (act >= 0 && bias != nullptr) ? bias[0] : 0.f;
    for (int64_t u0 = global_wave_id() * GPW; u0 < n_units; u0 += global_wave_count() * GPW) {
        const Unit un = unit_at(pl, u0 + grp);
        const int wave_len = wave_max_len<G>(un.len);
        Frag<VEC> xa = Frag<VEC>::zero();
        if (un.len > 0 && lig < dim_vec) {
            xa = Frag<VEC>::load(x + un.row * ld_x + lig * VEC);
            if (a != nullptr) xa = frag_mul(xa, Frag<VEC>::load(a + lig * VEC));
        }
        for (int base = 0; base < wave_len; base += G) {
            const bool have = base + lig < un.len;
            const int my_id = have ? pl.ids[un.begin + base + lig] : -1;
            float mine = 0.f;
#pragma unroll 1
            for (int j = 0; j < G; j += UNR) {
                if (base + j >= wave_len) break;                         // wave-uniform
                int id[UNR];
                Frag<VEC> row[UNR];
                float d[UNR];
#pragma unroll
                for (int k = 0; k < UNR; ++k) id[k] = __shfl(my_id, group_base + j + k);
#pragma unroll
                for (int k = 0; k < UNR; ++k)
                    row[k] = (id[k] >= 0 && lig < dim_vec) ? Frag<VEC>::load(y + static_cast<int64_t>(id[k]) * ld_y + lig * VEC) : Frag<VEC>::zero();
#pragma unroll
                for (int k = 0; k < UNR; ++k) d[k] = frag_dot(xa, row[k]);
                if (un.len > 0) {
                    // widths beyond one pass of the group (above 256, or above 64 on the 4-byte path): the further column chunks
                    for (int c = lig + G; c < dim_vec; c += G) {
                        Frag<VEC> xc = Frag<VEC>::load(x + un.row * ld_x + c * VEC);
                        if (a != nullptr) xc = frag_mul(xc, Frag<VEC>::load(a + c * VEC));
#pragma unroll
                        for (int k = 0; k < UNR; ++k)
                            if (id[k] >= 0) d[k] += frag_dot(xc, Frag<VEC>::load(y + static_cast<int64_t>(id[k]) * ld_y + c * VEC));
                    }
                }
#pragma unroll
                for (int k = 0; k < UNR; ++k) {
                    const float t = group_sum<G>(d[k]);
                    if (lig == j + k) mine = t;
                }
            }
            if (have) out[un.begin + base + lig] = act >= 0 ? gat_act(mine + c0, act) : mine;
        }
    }
}

__device__ __forceinline__ void merge_max_sum(float& m, float& l, float m2, float l2) {
    if (m2 == -__builtin_huge_valf()) return;
    const float mx = fmaxf(m, m2);
    l = l * expf(m - mx) + l2 * expf(m2 - mx);
    m = mx;
}

// ------------------------------------------------------------------------------------------------
// Softmax over every row (DGL edge_softmax, normalised per destination: GnnLayers.py:112).  Light rows are finished here; a segment of a split row leaves its
// (max, sum of m exp(z - max)) in partials[2 seg ..].  CONCAT: z[p] = act(src_term[STRIDE ids[p]] + dst_term[STRIDE v] + c) is formed (and stored) here (STRIDE 1: a
// plane per term, phase2.hip; 2: the two terms of a node side by side, gat.hip).  MULT: entry p
// stands for mult[ids[p]] copies with identical scores (phase2.hip's hyperedges kept once); without it no multiplicity is read.
// ------------------------------------------------------------------------------------------------
template <bool MULT>
__device__ __forceinline__ float softmax_weight(const float* __restrict__ mult, int id, float e) {
    if constexpr (MULT) return mult[id] * e;
    else return e;
}

template <bool CONCAT, bool MULT, int STRIDE>
__global__ __launch_bounds__(kBlockThreads) void attn_softmax_kernel(const float* __restrict__ src_term, const float* __restrict__ dst_term,
                                                                     const float* __restrict__ bias, const float* __restrict__ mult, int act, Plan pl,
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
            const float dst = un.len > 0 ? dst_term[STRIDE * un.row] + bias[0] : 0.f;
            for (int i = lig; i < un.len; i += G) {
                const int p = un.begin + i;
                const float v = gat_act(src_term[STRIDE * static_cast<int64_t>(pl.ids[p])] + dst, act);
                z[p] = v;
                m = fmaxf(m, v);
            }
        } else {
            for (int i = lig; i < un.len; i += G) m = fmaxf(m, z[un.begin + i]);
        }
        m = group_max<G>(m);
        float l = 0.f;
        for (int i = lig; i < un.len; i += G) l += softmax_weight<MULT>(mult, pl.ids[un.begin + i], expf(z[un.begin + i] - m));
        l = group_sum<G>(l);
        if (un.seg >= 0) {
            if (lig == 0) {
                partials[2 * un.seg] = m;
                partials[2 * un.seg + 1] = l;
            }
        } else if (un.row >= 0) {
            for (int i = lig; i < un.len; i += G) {
                const int p = un.begin + i;
                const float al = softmax_weight<MULT>(mult, pl.ids[p], expf(z[p] - m)) / l;
                alpha[p] = al;
                alpha_mirror[pl.mirror[p]] = al;
            }
        }
    }
}

// One workgroup per split row: merge its segments' (max, sum) in a fixed tree, then write alpha over the row's entries.
template <bool MULT>
__global__ __launch_bounds__(kBlockThreads) void attn_softmax_finish_kernel(Plan pl, const float* __restrict__ z, const float* __restrict__ mult,
                                                                            const float* __restrict__ partials, float* __restrict__ alpha,
                                                                            float* __restrict__ alpha_mirror) {
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
            const float al = softmax_weight<MULT>(mult, pl.ids[p], expf(z[p] - mx)) / den;
            alpha[p] = al;
            alpha_mirror[pl.mirror[p]] = al;
        }
    }
}

// block-wide sum in a fixed tree (thread order); every thread gets the result
__device__ __forceinline__ float block_sum(float v, float* red) {
    red[threadIdx.x] = v;
    __syncthreads();
    for (int o = kBlockThreads / 2; o > 0; o >>= 1) {
        if (static_cast<int>(threadIdx.x) < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    const float total = red[0];
    __syncthreads();
    return total;
}

// ------------------------------------------------------------------------------------------------
// Softmax backward: g holds d alpha on entry and ds (the gradient of the score BEFORE the activation) on return:
//   ds[p] = alpha[p] (g[p] - c_v) act'(z[p]),  c_v = sum over row v of alpha g.   node_sums[2 v + 1] = sum over row v of ds (v as the destination).
// Two things keep the row's cancellation out of the result:
//   * g is taken relative to the row's first entry g0:  g - c_v = (g - g0) - sum alpha (g - g0).  Where a row's d alpha are nearly equal (smooth features),
//     c_v formed from the raw values carries eps |c_v| of rounding, far more than the spread g - c_v that ds is made of.
//   * with t = alpha (g - c_v), sum t = 0 (alpha sums to one), so  sum t a = - sum t (1 - a)  (a = act'): the row sum takes the form whose alpha-mass is smaller -
//     exactly 0 for a row whose scores all have a = 1 (or all a = 0), as in exact arithmetic, instead of eps sum |t| of noise in the input gradient and d c.
// ------------------------------------------------------------------------------------------------
struct RowBwd {
    float ma, mb, sa, sb;                 // sum alpha a, sum alpha (1 - a), sum t a, sum t (1 - a)
    __device__ float row_sum() const { return mb < ma ? -sb : sa; }
};

__device__ __forceinline__ void ds_entry(const float* __restrict__ z, const float* __restrict__ alpha, float* __restrict__ g, int act, int p, float g0, float c,
                                         RowBwd& r) {
    const float a = gat_act_grad(z[p], act);
    const float al = alpha[p];
    const float t = al * ((g[p] - g0) - c);
    g[p] = t * a;
    r.ma += al * a;
    r.mb += al * (1.f - a);
    r.sa += t * a;
    r.sb += t * (1.f - a);
}

__global__ __launch_bounds__(kBlockThreads) void gat_softmax_bwd_kernel(const float* __restrict__ z, const float* __restrict__ alpha, float* __restrict__ g, int act,
                                                                        Plan pl, float* __restrict__ node_sums, float* __restrict__ partials) {
    constexpr int G = kScalarLanes, GPW = kWave / G;
    const int lane = threadIdx.x & (kWave - 1);
    const int lig = lane & (G - 1);
    const int grp = lane / G;
    const int64_t n_units = pl.n_segments + pl.n_rows;
    for (int64_t u0 = global_wave_id() * GPW; u0 < n_units; u0 += global_wave_count() * GPW) {
        const Unit un = unit_at(pl, u0 + grp);
        const float g0 = un.len > 0 ? g[pl.rowptr[un.row]] : 0.f;      // (read by every lane before any lane of this row writes)
        float c = 0.f;
        for (int i = lig; i < un.len; i += G) c += alpha[un.begin + i] * (g[un.begin + i] - g0);
        c = group_sum<G>(c);
        RowBwd r{0.f, 0.f, 0.f, 0.f};
        if (un.seg < 0 && un.row >= 0)
            for (int i = lig; i < un.len; i += G) ds_entry(z, alpha, g, act, un.begin + i, g0, c, r);
        r.ma = group_sum<G>(r.ma);
        r.mb = group_sum<G>(r.mb);
        r.sa = group_sum<G>(r.sa);
        r.sb = group_sum<G>(r.sb);
        if (lig == 0) {
            if (un.seg >= 0) partials[un.seg] = c;
            else if (un.row >= 0) node_sums[2 * un.row + 1] = r.row_sum();
        }
    }
}

__global__ __launch_bounds__(kBlockThreads) void gat_softmax_bwd_finish_kernel(const float* __restrict__ z, const float* __restrict__ alpha, float* __restrict__ g, int act,
                                                                               Plan pl, float* __restrict__ node_sums, const float* __restrict__ partials) {
    __shared__ float red[kBlockThreads];
    const int t = threadIdx.x;
    for (int64_t hr = blockIdx.x; hr < pl.n_heavy; hr += gridDim.x) {
        const int64_t row = pl.heavy_rows[hr];
        const float g0 = g[pl.rowptr[row]];                                 // (block_sum's barriers order this read before the writes below)
        const int s0 = pl.heavy_segptr[hr], s1 = pl.heavy_segptr[hr + 1];
        float c = 0.f;
        for (int sg = s0 + t; sg < s1; sg += kBlockThreads) c += partials[sg];
        c = block_sum(c, red);
        RowBwd r{0.f, 0.f, 0.f, 0.f};
        for (int p = pl.rowptr[row] + t; p < pl.rowptr[row + 1]; p += kBlockThreads) ds_entry(z, alpha, g, act, p, g0, c, r);
        r.ma = block_sum(r.ma, red);
        r.mb = block_sum(r.mb, red);
        r.sa = block_sum(r.sa, red);
        r.sb = block_sum(r.sb, red);
        if (t == 0) node_sums[2 * row + 1] = r.row_sum();
    }
}

// dh[v] (+)= [node_sums[2 v] w_src +] node_sums[2 v + 1] w_dst (concat)   |   dh[v] (+)= w * b[v] (product).  ACCUM: dh holds the transposed aggregation on entry
// (gat.hip); SRC: v is also the source of edges (gat.hip; in phase2.hip the sources are the hyperedge rows)
template <int VEC, bool ACCUM, bool SRC>
__global__ __launch_bounds__(kBlockThreads) void attn_node_grad_kernel(float* __restrict__ dh, int64_t ld_dh, const float* __restrict__ b, int64_t ld_b,
                                                                       const float* __restrict__ node_sums, const float* __restrict__ w, int head, int64_t n_rows,
                                                                       int dim, int dim_vec) {
    const int64_t total = n_rows * dim_vec;
    for (int64_t i = static_cast<int64_t>(blockIdx.x) * kBlockThreads + threadIdx.x; i < total; i += static_cast<int64_t>(gridDim.x) * kBlockThreads) {
        const int64_t r = i / dim_vec;
        const int c = static_cast<int>(i - r * dim_vec);
        Frag<VEC> acc = Frag<VEC>::zero();
        if constexpr (ACCUM) acc = Frag<VEC>::load(dh + r * ld_dh + c * VEC);
        if (head == IHG_GAT_CONCAT) {
            Frag<VEC> t = Frag<VEC>::zero();
            if constexpr (SRC) t.add_scaled(Frag<VEC>::load(w + c * VEC), node_sums[2 * r]);
            t.add_scaled(Frag<VEC>::load(w + dim + c * VEC), node_sums[2 * r + 1]);
            if constexpr (ACCUM) acc.add(t);
            else acc = t;
        } else {
            const Frag<VEC> t = frag_mul(Frag<VEC>::load(w + c * VEC), Frag<VEC>::load(b + r * ld_b + c * VEC));
            if constexpr (ACCUM) acc.add(t);
            else acc = t;
        }
        acc.store(dh + r * ld_dh + c * VEC);
    }
}

// ------------------------------------------------------------------------------------------------
// Launch helpers
// ------------------------------------------------------------------------------------------------
inline int gat_grid(int64_t waves) {
    int64_t blocks = (waves + kWavesPerBlock - 1) / kWavesPerBlock;
    if (blocks < 1) blocks = 1;
    if (blocks > kMaxBlocks * 4) blocks = kMaxBlocks * 4;
    return static_cast<int>(blocks);
}

// n units, one per group of G lanes
inline int group_grid(int64_t n, int G) { return gat_grid((n + kWave / G - 1) / (kWave / G)); }

inline int scalar_grid(const Plan& pl) { return group_grid(pl.n_segments + pl.n_rows, kScalarLanes); }

inline int flat_grid(int64_t n) {
    const int64_t blocks = (n + kBlockThreads - 1) / kBlockThreads;
    return static_cast<int>(std::max<int64_t>(1, std::min<int64_t>(blocks, kMaxBlocks * 4)));
}

template <int W>
void launch_project(bool vec4, const float* x, int64_t ld_x, const float* w, int dim, int64_t n_rows, float* out, hipStream_t s) {
    with_row_lanes(vec4, dim, [&](auto vec, auto g) {
        constexpr int VEC = decltype(vec)::value, G = decltype(g)::value;
        hipLaunchKernelGGL((attn_project_kernel<VEC, G, W>), dim3(group_grid(n_rows, G)), dim3(kBlockThreads), 0, s, x, ld_x, w, dim, dim / VEC, n_rows, out);
    });
}

void launch_row_dot(bool vec4, const float* x, int64_t ld_x, const float* a, const float* y, int64_t ld_y, const float* bias, int act, const Plan& pl, int dim,
                    float* out, hipStream_t s) {
    with_row_lanes(vec4, dim, [&](auto vec, auto g) {
        constexpr int VEC = decltype(vec)::value, G = decltype(g)::value;
        hipLaunchKernelGGL((gat_row_dot_kernel<VEC, G>), dim3(group_grid(pl.n_segments + pl.n_rows, G)), dim3(kBlockThreads), 0, s, x, ld_x, a, y, ld_y, bias, act, pl,
                           dim / VEC, out);
    });
}

// the softmax over every row and, where the plan has split rows, their finish
template <bool CONCAT, bool MULT, int STRIDE = 1>
void launch_softmax(const float* src_term, const float* dst_term, const float* bias, const float* mult, int act, const Plan& pl, float* z, float* alpha,
                    float* alpha_mirror, float* partials, hipStream_t s) {
    hipLaunchKernelGGL((attn_softmax_kernel<CONCAT, MULT, STRIDE>), dim3(scalar_grid(pl)), dim3(kBlockThreads), 0, s, src_term, dst_term, bias, mult, act, pl, z, alpha,
                       alpha_mirror, partials);
    if (pl.n_heavy > 0)
        hipLaunchKernelGGL(attn_softmax_finish_kernel<MULT>, dim3(heavy_grid(pl.n_heavy)), dim3(kBlockThreads), 0, s, pl, z, mult, partials, alpha, alpha_mirror);
}

void launch_softmax_bwd(const float* z, const float* alpha, float* g, int act, const Plan& pl, float* node_sums, float* partials, hipStream_t s) {
    hipLaunchKernelGGL(gat_softmax_bwd_kernel, dim3(scalar_grid(pl)), dim3(kBlockThreads), 0, s, z, alpha, g, act, pl, node_sums, partials);
    if (pl.n_heavy > 0)
        hipLaunchKernelGGL(gat_softmax_bwd_finish_kernel, dim3(heavy_grid(pl.n_heavy)), dim3(kBlockThreads), 0, s, z, alpha, g, act, pl, node_sums, partials);
}

template <bool ACCUM, bool SRC>
void launch_node_grad(bool vec4, float* dh, int64_t ld_dh, const float* b, int64_t ld_b, const float* node_sums, const float* w, int head, int64_t n_rows, int dim,
                      hipStream_t s) {
    if (vec4)
        hipLaunchKernelGGL((attn_node_grad_kernel<4, ACCUM, SRC>), dim3(flat_grid(n_rows * (dim / 4))), dim3(kBlockThreads), 0, s, dh, ld_dh, b, ld_b, node_sums, w, head,
                           n_rows, dim, dim / 4);
    else
        hipLaunchKernelGGL((attn_node_grad_kernel<1, ACCUM, SRC>), dim3(flat_grid(n_rows * dim)), dim3(kBlockThreads), 0, s, dh, ld_dh, b, ld_b, node_sums, w, head, n_rows,
                           dim, dim);
}

int64_t param_blocks(int64_t n_rows) { return std::max<int64_t>(1, (n_rows + kParamRows - 1) / kParamRows); }

// ------------------------------------------------------------------------------------------------
// Entry-point checks (`what`: the entry point's name, as its messages carry it)
// ------------------------------------------------------------------------------------------------
int check_head(const char* what, int32_t head) {
    if (head != IHG_GAT_CONCAT && head != IHG_GAT_PRODUCT) return fail(IHG_ERR_INVALID, "%s: unknown head %d", what, head);
    return IHG_OK;
}

int check_plan(const char* what, const Plan& pl, int32_t head, int32_t activation, int32_t dim) {
    if (pl.n_rows < 0 || dim <= 0 || pl.n_segments < 0 || pl.n_heavy < 0) return fail(IHG_ERR_INVALID, "%s: bad size (rows=%lld dim=%d)", what, (long long)pl.n_rows, dim);
    if (const int rc = check_head(what, head); rc != IHG_OK) return rc;
    if (activation != IHG_GAT_LEAKY_RELU && activation != IHG_GAT_RELU && activation != IHG_GAT_TANH) return fail(IHG_ERR_INVALID, "%s: unknown activation %d", what, activation);
    if (pl.n_rows > 0 && (pl.rowptr == nullptr || pl.ids == nullptr || pl.mirror == nullptr)) return fail(IHG_ERR_INVALID, "%s: null graph pointer", what);
    return check_split_rows(what, pl, true);
}

int check_pointers(const char* what, std::initializer_list<const void*> pointers) {
    for (const void* p : pointers)
        if (p == nullptr) return fail(IHG_ERR_INVALID, "%s: null pointer", what);
    return IHG_OK;
}

int check_workspace(const char* what, int64_t have, int64_t need) {
    if (have < need) return fail(IHG_ERR_WORKSPACE, "%s: workspace %lld < %lld bytes", what, (long long)have, (long long)need);
    return IHG_OK;
}

}  // namespace
