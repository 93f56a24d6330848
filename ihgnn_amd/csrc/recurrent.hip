// recurrent.hip - the GRU query encoder (Gs.Query.transform == 'gru'): X0[query] = the last hidden state of a one-layer GRU over the rows of the query's words, in
// file order, h_0 = 0 (torch.nn.GRU's arithmetic, gates r, z, n).  fp32 throughout: every matrix product runs on v_mfma_f32_16x16x4_f32.
//
//   gru_fwd_kernel         one workgroup per tile of 32 bags that are adjacent in the length-sorted order; the workgroup runs its OWN time loop to its longest member
//                          and masks the finished bags - one launch whatever the longest bag is, no grid-wide step.  h [32, d] lives in LDS; x_t is gathered from the
//                          table as the A operand; W_ih / W_hh (6 d^2 floats, 96 KiB at d = 64, 1.5 MiB at d = 256) are streamed from L2 per step at every width as the
//                          B operand (16 B per lane: the k order inside a 16-wide chunk is permuted the same way for A and B).  With `saved`: r, z, n, W_hn h + b_hn
//                          and h_{t-1} per word occurrence (5 W d floats).
//   gru_bwd_steps_kernel   the same tiles backwards in time: dh [32, d] in LDS, per step the four pre-activation gradients [dr, dz, dn, dn * r] of the occurrence into the
//                          workspace (dg [W, 4 d]), then dh += [dr dz dn*r] W_hh and dx[p] = [dr dz dn] W_ih on the matrix cores (dx [W, d])
//   gru_wgrad_kernel       dW_ih = dgi^T x, dW_hh = dgh^T h_prev, db = dg^T 1 over fixed slabs of occurrences (a 64 x 32 output tile per workgroup, its four waves take the
//                          slab's 16-row chunks round-robin and are added in wave order)
//   gru_finish_kernel      the slabs added in slab order
// and d_table = the K7 segment sum of dx over every word's positions (ihg_node_segment_sum).  No float atomics anywhere: two runs give the same bits.
#include "common.hpp"

namespace {

constexpr int kGruTile = 32;          // bags per workgroup
constexpr int kGruMaxSlabs = 32;
constexpr int kGruSlabRows = 2048;    // occurrences per slab before the slab count saturates

inline int gru_slabs(int64_t n_words) { return static_cast<int>(std::max<int64_t>(1, std::min<int64_t>(kGruMaxSlabs, (n_words + kGruSlabRows - 1) / kGruSlabRows))); }
inline int64_t gru_slab_len(int64_t n_words) {
    const int64_t s = gru_slabs(n_words);
    return ((n_words + s - 1) / s + 63) / 64 * 64;
}
inline int64_t gru_slab_floats(int dim) { return 2 * (3 * static_cast<int64_t>(dim) * dim + 3 * dim); }

struct GruWorkspace {
    float* dg;        // [W, 4 d]
    float* dx;        // [W, d]
    float* slabs;     // [slabs][2][3 d d + 3 d]
};
inline int64_t gru_workspace_floats(int64_t n_words, int dim) {
    return n_words * 5 * dim + gru_slabs(n_words) * gru_slab_floats(dim);
}
inline GruWorkspace gru_carve(void* workspace, int64_t n_words, int dim) {
    float* p = static_cast<float*>(workspace);
    return {p, p + n_words * 4 * dim, p + n_words * 5 * dim};
}

struct GruTiles {
    const int32_t* bag_ptr;
    const int32_t* words;
    const int32_t* order;     // bags by decreasing length (nullptr: as they are)
    int64_t n_bags;
};

struct GruFwd {
    const float* table;
    int64_t ld_table;
    GruTiles t;
    const float *w_ih, *w_hh, *b_ih, *b_hh;
    float* out;
    int64_t ld_out;
    float* saved;
};

struct GruBwd {
    const float* d_query;
    int64_t ld_dq;
    GruTiles t;
    const float *w_ih, *w_hh;
    const float* saved;
    float* dg;
    float* dx;
};

struct GruWgrad {
    const float* table;
    int64_t ld_table;
    const int32_t* words;
    const float* saved;
    const float* dg;
    int64_t n_words, slab_len;
    float* slabs;
};

__device__ __forceinline__ float sigmoidf(float x) { return 1.f / (1.f + expf(-x)); }

// the tile's bags into LDS (bag id or -1, first word position, length) and its longest length; ends with a barrier
__device__ __forceinline__ int gru_load_tile(const GruTiles& t, int64_t tile, int* s_bag, int* s_ptr, int* s_len, int* s_max) {
    const int tid = threadIdx.x;
    if (tid == 0) *s_max = 0;
    if (tid < kGruTile) {
        const int64_t idx = tile * kGruTile + tid;
        int bag = -1, p0 = 0, len = 0;
        if (idx < t.n_bags) {
            bag = t.order != nullptr ? t.order[idx] : static_cast<int>(idx);
            p0 = t.bag_ptr[bag];
            len = t.bag_ptr[bag + 1] - p0;
        }
        s_bag[tid] = bag, s_ptr[tid] = p0, s_len[tid] = len;
    }
    __syncthreads();
    if (tid < kGruTile) atomicMax(s_max, s_len[tid]);
    __syncthreads();
    return *s_max;
}

template <int D>
__global__ __launch_bounds__(kBlockThreads) void gru_fwd_kernel(GruFwd a, int64_t n_tiles) {
    constexpr int MT = kGruTile, HS = D + kRowPad, CB = D / 16, CPW = (CB + kWavesPerBlock - 1) / kWavesPerBlock;
    __shared__ __attribute__((aligned(16))) float h[MT][HS];
    __shared__ int s_bag[MT], s_ptr[MT], s_len[MT], s_max;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n = lane & 15, kq = lane >> 4;
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        __syncthreads();
        const int steps = gru_load_tile(a.t, tile, s_bag, s_ptr, s_len, &s_max);
        for (int e = tid; e < MT * D; e += kBlockThreads) h[e / D][e % D] = 0.f;
        __syncthreads();
        for (int t = 0; t < steps; ++t) {
            v4f h_new[CPW][2];
            const float* xrow[2];
#pragma unroll
            for (int ms = 0; ms < 2; ++ms) {
                const int m = ms * 16 + n;
                xrow[ms] = t < s_len[m] ? a.table + static_cast<int64_t>(a.t.words[s_ptr[m] + t]) * a.ld_table : nullptr;
            }
#pragma unroll
            for (int j = 0; j < CPW; ++j) {
                const int cb = wave + j * kWavesPerBlock;
                if (cb >= CB) continue;
                v4f acc[2][4];
#pragma unroll
                for (int ms = 0; ms < 2; ++ms)
#pragma unroll
                    for (int g = 0; g < 4; ++g) acc[ms][g] = v4f{0.f, 0.f, 0.f, 0.f};
                const int64_t wrow = static_cast<int64_t>(cb * 16 + n) * D + kq * 4;      // B[k][n] = W[gate * D + cb * 16 + n][k]
#pragma unroll 2
                for (int k0 = 0; k0 < D / 16; ++k0) {
                    const int kk = k0 * 16;
                    v4f bi[3], bh[3];
#pragma unroll
                    for (int g = 0; g < 3; ++g) {
                        bi[g] = *reinterpret_cast<const v4f*>(a.w_ih + static_cast<int64_t>(g) * D * D + wrow + kk);
                        bh[g] = *reinterpret_cast<const v4f*>(a.w_hh + static_cast<int64_t>(g) * D * D + wrow + kk);
                    }
#pragma unroll
                    for (int ms = 0; ms < 2; ++ms) {
                        const v4f ax = xrow[ms] != nullptr ? *reinterpret_cast<const v4f*>(xrow[ms] + kk + kq * 4) : v4f{0.f, 0.f, 0.f, 0.f};
                        const v4f ah = *reinterpret_cast<const v4f*>(&h[ms * 16 + n][kk + kq * 4]);
#pragma unroll
                        for (int i = 0; i < 4; ++i) {
                            acc[ms][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(ax[i], bi[0][i], acc[ms][0], 0, 0, 0);
                            acc[ms][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(ax[i], bi[1][i], acc[ms][1], 0, 0, 0);
                            acc[ms][2] = __builtin_amdgcn_mfma_f32_16x16x4f32(ax[i], bi[2][i], acc[ms][2], 0, 0, 0);
                            acc[ms][3] = __builtin_amdgcn_mfma_f32_16x16x4f32(ah[i], bh[2][i], acc[ms][3], 0, 0, 0);
                        }
#pragma unroll
                        for (int i = 0; i < 4; ++i) {
                            acc[ms][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(ah[i], bh[0][i], acc[ms][0], 0, 0, 0);
                            acc[ms][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(ah[i], bh[1][i], acc[ms][1], 0, 0, 0);
                        }
                    }
                }
                // the gates of this lane's column c, rows ms * 16 + 4 kq + i
                const int c = cb * 16 + n;
                const float b_r = a.b_ih[c] + a.b_hh[c], b_z = a.b_ih[D + c] + a.b_hh[D + c], b_in = a.b_ih[2 * D + c], b_hn = a.b_hh[2 * D + c];
#pragma unroll
                for (int ms = 0; ms < 2; ++ms)
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int m = ms * 16 + 4 * kq + i;
                        const float hp = h[m][c];
                        const float r = sigmoidf(acc[ms][0][i] + b_r), z = sigmoidf(acc[ms][1][i] + b_z);
                        const float hn = acc[ms][3][i] + b_hn;
                        const float nn = tanhf(acc[ms][2][i] + b_in + r * hn);
                        h_new[j][ms][i] = (1.f - z) * nn + z * hp;
                        if (a.saved != nullptr && t < s_len[m]) {
                            float* sv = a.saved + static_cast<int64_t>(s_ptr[m] + t) * 5 * D + c;
                            sv[0] = r, sv[D] = z, sv[2 * D] = nn, sv[3 * D] = hn, sv[4 * D] = hp;
                        }
                    }
            }
            __syncthreads();      // every wave has read h_{t-1}
#pragma unroll
            for (int j = 0; j < CPW; ++j) {
                const int cb = wave + j * kWavesPerBlock;
                if (cb >= CB) continue;
#pragma unroll
                for (int ms = 0; ms < 2; ++ms)
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int m = ms * 16 + 4 * kq + i;
                        if (t < s_len[m]) h[m][cb * 16 + n] = h_new[j][ms][i];
                    }
            }
            __syncthreads();
        }
        for (int e = tid; e < MT * D; e += kBlockThreads) {
            const int m = e / D, c = e % D;
            if (s_bag[m] >= 0) a.out[static_cast<int64_t>(s_bag[m]) * a.ld_out + c] = h[m][c];
        }
    }
}

template <int D>
__global__ __launch_bounds__(kBlockThreads) void gru_bwd_steps_kernel(GruBwd a, int64_t n_tiles) {
    constexpr int MT = kGruTile, HS = D + kRowPad, CB = D / 16, CPW = (CB + kWavesPerBlock - 1) / kWavesPerBlock;
    __shared__ __attribute__((aligned(16))) float dh[MT][HS];
    __shared__ int s_bag[MT], s_ptr[MT], s_len[MT], s_max;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n = lane & 15, kq = lane >> 4;
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        __syncthreads();
        const int steps = gru_load_tile(a.t, tile, s_bag, s_ptr, s_len, &s_max);
        for (int e = tid; e < MT * D; e += kBlockThreads) {
            const int m = e / D, c = e % D;
            dh[m][c] = s_bag[m] >= 0 && s_len[m] > 0 ? a.d_query[static_cast<int64_t>(s_bag[m]) * a.ld_dq + c] : 0.f;
        }
        __syncthreads();
        for (int t = steps - 1; t >= 0; --t) {
            // the gates' pre-activation gradients of every live occurrence of this step; dh keeps its direct part dh * z
            for (int e = tid; e < MT * D; e += kBlockThreads) {
                const int m = e / D, c = e % D;
                if (t >= s_len[m]) continue;
                const int64_t p = s_ptr[m] + t;
                const float* sv = a.saved + p * 5 * D + c;
                const float r = sv[0], z = sv[D], nn = sv[2 * D], hn = sv[3 * D], hp = sv[4 * D];
                const float g = dh[m][c];
                const float dnp = g * (1.f - z) * (1.f - nn * nn);
                float* dg = a.dg + p * 4 * D + c;
                dg[0] = dnp * hn * (r * (1.f - r));
                dg[D] = g * (hp - nn) * (z * (1.f - z));
                dg[2 * D] = dnp;
                dg[3 * D] = dnp * r;
                dh[m][c] = g * z;
            }
            __syncthreads();
            const float* grow[2];
#pragma unroll
            for (int ms = 0; ms < 2; ++ms) {
                const int m = ms * 16 + n;
                grow[ms] = t < s_len[m] ? a.dg + static_cast<int64_t>(s_ptr[m] + t) * 4 * D + kq * 4 : nullptr;
            }
#pragma unroll 1
            for (int j = 0; j < CPW; ++j) {
                const int cb = wave + j * kWavesPerBlock;
                if (cb >= CB) continue;
                const int c = cb * 16 + n;
                v4f acc_h[2], acc_x[2];
#pragma unroll
                for (int ms = 0; ms < 2; ++ms) acc_h[ms] = acc_x[ms] = v4f{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int g = 0; g < 3; ++g) {
#pragma unroll 2
                    for (int k0 = 0; k0 < D / 16; ++k0) {
                        const int kk = k0 * 16;
                        const int64_t wr = (static_cast<int64_t>(g) * D + kk + kq * 4) * D + c;      // B[k][n] = W[gate * D + k][c]
                        v4f bx, bh;
#pragma unroll
                        for (int i = 0; i < 4; ++i) bx[i] = a.w_ih[wr + static_cast<int64_t>(i) * D], bh[i] = a.w_hh[wr + static_cast<int64_t>(i) * D];
#pragma unroll
                        for (int ms = 0; ms < 2; ++ms) {
                            const v4f zero = v4f{0.f, 0.f, 0.f, 0.f};
                            const v4f ai = grow[ms] != nullptr ? *reinterpret_cast<const v4f*>(grow[ms] + g * D + kk) : zero;
                            const v4f ah = g < 2 ? ai : (grow[ms] != nullptr ? *reinterpret_cast<const v4f*>(grow[ms] + 3 * D + kk) : zero);
#pragma unroll
                            for (int i = 0; i < 4; ++i) {
                                acc_x[ms] = __builtin_amdgcn_mfma_f32_16x16x4f32(ai[i], bx[i], acc_x[ms], 0, 0, 0);
                                acc_h[ms] = __builtin_amdgcn_mfma_f32_16x16x4f32(ah[i], bh[i], acc_h[ms], 0, 0, 0);
                            }
                        }
                    }
                }
#pragma unroll
                for (int ms = 0; ms < 2; ++ms)
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int m = ms * 16 + 4 * kq + i;
                        if (t < s_len[m]) {
                            dh[m][c] += acc_h[ms][i];
                            a.dx[static_cast<int64_t>(s_ptr[m] + t) * D + c] = acc_x[ms][i];
                        }
                    }
            }
            __syncthreads();
        }
    }
}

// grid (output tiles, slabs, 2): tile = 64 rows c of the [3 D, D] gradient x 32 columns j; z = 0: dW_ih / db_ih (dg's dn, the words' table rows), 1: dW_hh / db_hh
// (dg's dn * r, the saved h_{t-1})
template <int D>
__global__ __launch_bounds__(kBlockThreads) void gru_wgrad_kernel(GruWgrad a) {
    constexpr int JT = D / 32;
    __shared__ float red[kWavesPerBlock][64][33];
    __shared__ float red_b[kWavesPerBlock][64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n = lane & 15, kq = lane >> 4;
    const int ct = blockIdx.x / JT, jt = blockIdx.x % JT, which = blockIdx.z;
    const int64_t p_begin = static_cast<int64_t>(blockIdx.y) * a.slab_len, p_end = p_begin + a.slab_len < a.n_words ? p_begin + a.slab_len : a.n_words;
    int col_a[4];
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
        const int c = ct * 64 + mt * 16 + n, g = c / D, cc = c - g * D;
        col_a[mt] = c >= 3 * D ? -1 : (g < 2 ? g * D : (which ? 3 * D : 2 * D)) + cc;      // (3 D = 96 rows at D = 32: the second tile is part-filled)
    }
    v4f acc[4][2], acc_b[4];
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) acc[mt][0] = acc[mt][1] = acc_b[mt] = v4f{0.f, 0.f, 0.f, 0.f};
    for (int64_t p0 = p_begin + wave * 16; p0 < p_end; p0 += 16 * kWavesPerBlock) {
        float av[4][4], bv[2][4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int64_t p = p0 + kq * 4 + i;
            const bool live = p < p_end;
            const float* src = nullptr;
            if (live) src = which ? a.saved + p * 5 * D + 4 * D : a.table + static_cast<int64_t>(a.words[p]) * a.ld_table;
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) av[mt][i] = live && col_a[mt] >= 0 ? a.dg[p * 4 * D + col_a[mt]] : 0.f;
#pragma unroll
            for (int nt = 0; nt < 2; ++nt) bv[nt][i] = live ? src[jt * 32 + nt * 16 + n] : 0.f;
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) {
                acc[mt][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[mt][i], bv[0][i], acc[mt][0], 0, 0, 0);
                acc[mt][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[mt][i], bv[1][i], acc[mt][1], 0, 0, 0);
                if (jt == 0) acc_b[mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[mt][i], 1.f, acc_b[mt], 0, 0, 0);
            }
    }
#pragma unroll
    for (int mt = 0; mt < 4; ++mt)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int row = mt * 16 + 4 * kq + i;
            red[wave][row][n] = acc[mt][0][i];
            red[wave][row][16 + n] = acc[mt][1][i];
            if (n == 0) red_b[wave][row] = acc_b[mt][i];
        }
    __syncthreads();
    float* slab = a.slabs + (static_cast<int64_t>(blockIdx.y) * 2 + which) * (3 * D * D + 3 * D);
    for (int e = tid; e < 64 * 32; e += kBlockThreads) {
        const int row = e >> 5, col = e & 31;
        if (ct * 64 + row < 3 * D) slab[static_cast<int64_t>(ct * 64 + row) * D + jt * 32 + col] = (red[0][row][col] + red[1][row][col]) + (red[2][row][col] + red[3][row][col]);
    }
    if (jt == 0 && tid < 64 && ct * 64 + tid < 3 * D) slab[3 * D * D + ct * 64 + tid] = (red_b[0][tid] + red_b[1][tid]) + (red_b[2][tid] + red_b[3][tid]);
}

__global__ __launch_bounds__(kBlockThreads) void gru_finish_kernel(const float* __restrict__ slabs, int n_slabs, int dim, float* __restrict__ dw_ih, float* __restrict__ dw_hh,
                                                                   float* __restrict__ db_ih, float* __restrict__ db_hh) {
    const int64_t mat = 3 * static_cast<int64_t>(dim) * dim, per = mat + 3 * dim;
    for (int64_t idx = static_cast<int64_t>(blockIdx.x) * kBlockThreads + threadIdx.x; idx < 2 * per; idx += static_cast<int64_t>(gridDim.x) * kBlockThreads) {
        float sum = 0.f;
        for (int s = 0; s < n_slabs; ++s) sum += slabs[static_cast<int64_t>(s) * 2 * per + idx];
        const int which = idx >= per;
        const int64_t e = idx - which * per;
        if (e < mat) (which ? dw_hh : dw_ih)[e] = sum;
        else (which ? db_hh : db_ih)[e - mat] = sum;
    }
}

template <int D>
void launch_gru_fwd(const GruFwd& a, hipStream_t s) {
    const int64_t tiles = (a.t.n_bags + kGruTile - 1) / kGruTile;
    hipLaunchKernelGGL(gru_fwd_kernel<D>, dim3(static_cast<unsigned>(std::min<int64_t>(tiles, kMaxBlocks))), dim3(kBlockThreads), 0, s, a, tiles);
}

template <int D>
void launch_gru_bwd(const GruBwd& a, const GruWgrad& g, float* dw_ih, float* dw_hh, float* db_ih, float* db_hh, hipStream_t s) {
    const int64_t tiles = (a.t.n_bags + kGruTile - 1) / kGruTile;
    const int slabs = gru_slabs(g.n_words);
    hipLaunchKernelGGL(gru_bwd_steps_kernel<D>, dim3(static_cast<unsigned>(std::min<int64_t>(tiles, kMaxBlocks))), dim3(kBlockThreads), 0, s, a, tiles);
    hipLaunchKernelGGL(gru_wgrad_kernel<D>, dim3(((3 * D + 63) / 64) * (D / 32), slabs, 2), dim3(kBlockThreads), 0, s, g);
    const int64_t total = gru_slab_floats(D);
    hipLaunchKernelGGL(gru_finish_kernel, dim3(static_cast<unsigned>(std::min<int64_t>((total + kBlockThreads - 1) / kBlockThreads, kMaxBlocks))), dim3(kBlockThreads), 0, s,
                       g.slabs, slabs, D, dw_ih, dw_hh, db_ih, db_hh);
}

}  // namespace

extern "C" {

int64_t ihg_gru_workspace_bytes(int64_t n_bags, int64_t n_words, int32_t dim) {
    if (dim < 1 || dim > 256 || n_bags < 0 || n_words < 0) return -1;
    int d = 32;
    while (d < dim) d *= 2;
    return std::max<int64_t>(16, gru_workspace_floats(n_words, d) * 4);
}

int64_t ihg_gru_saved_bytes(int64_t n_words, int32_t dim) {
    if (dim < 1 || dim > 256 || n_words < 0) return -1;
    int d = 32;
    while (d < dim) d *= 2;
    return std::max<int64_t>(16, n_words * 5 * d * 4);
}

int ihg_gru_fwd(const float* table, int64_t ld_table, const int32_t* bag_ptr, const int32_t* words, const int32_t* bag_order, int64_t n_bags, int64_t n_words,
                const float* w_ih, const float* w_hh, const float* b_ih, const float* b_hh, float* out, int64_t ld_out, float* saved, void* workspace,
                int64_t workspace_bytes, int32_t dim, ihg_stream_t stream) {
    const char* what = "ihg_gru_fwd";
    (void)workspace;
    if (!mfma_dim(dim)) return fail(IHG_ERR_INVALID, "%s: dim %d is not one of 32 / 64 / 128 / 256 (pad the operands with zeros)", what, dim);
    if (n_bags < 0 || n_words < 0 || n_words > INT32_MAX || ld_table < dim || ld_table % 4 != 0 || ld_out < dim || workspace_bytes < 0)
        return fail(IHG_ERR_INVALID, "%s: bad size (bags=%lld words=%lld ld_table=%lld ld_out=%lld)", what, (long long)n_bags, (long long)n_words, (long long)ld_table,
                    (long long)ld_out);
    if (n_bags == 0) return IHG_OK;
    if (bag_ptr == nullptr || out == nullptr) return fail(IHG_ERR_INVALID, "%s: null bag_ptr or out", what);
    if (n_words > 0 && (table == nullptr || words == nullptr || w_ih == nullptr || w_hh == nullptr || b_ih == nullptr || b_hh == nullptr))
        return fail(IHG_ERR_INVALID, "%s: null table, words or parameter", what);
    if (n_words > 0 && (!aligned16(table) || !aligned16(w_ih) || !aligned16(w_hh))) return fail(IHG_ERR_INVALID, "%s: table, w_ih and w_hh must be 16-byte aligned", what);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const GruFwd a{table, ld_table, {bag_ptr, words, bag_order, n_bags}, w_ih, w_hh, b_ih, b_hh, out, ld_out, saved};
    switch (dim) {
        case 32: launch_gru_fwd<32>(a, s); break;
        case 64: launch_gru_fwd<64>(a, s); break;
        case 128: launch_gru_fwd<128>(a, s); break;
        default: launch_gru_fwd<256>(a, s); break;
    }
    return check_launch(what);
}

int ihg_gru_bwd(const float* d_query, int64_t ld_dq, const float* table, int64_t ld_table, const int32_t* bag_ptr, const int32_t* words, const int32_t* bag_order,
                int64_t n_bags, int64_t n_words, const int32_t* word_ptr, const int32_t* word_pos, int64_t n_table_rows, const float* w_ih, const float* w_hh,
                const float* saved, float* d_table, float* dw_ih, float* dw_hh, float* db_ih, float* db_hh, void* workspace,
                int64_t workspace_bytes, int32_t dim, ihg_stream_t stream) {
    const char* what = "ihg_gru_bwd";
    if (!mfma_dim(dim)) return fail(IHG_ERR_INVALID, "%s: dim %d is not one of 32 / 64 / 128 / 256 (pad the operands with zeros)", what, dim);
    if (n_bags < 0 || n_words < 0 || n_words > INT32_MAX || n_table_rows < 0 || ld_table < dim || ld_table % 4 != 0 || ld_dq < dim)
        return fail(IHG_ERR_INVALID, "%s: bad size (bags=%lld words=%lld rows=%lld ld_table=%lld ld_dq=%lld)", what, (long long)n_bags, (long long)n_words,
                    (long long)n_table_rows, (long long)ld_table, (long long)ld_dq);
    if (dw_ih == nullptr || dw_hh == nullptr || db_ih == nullptr || db_hh == nullptr || (d_table == nullptr && n_table_rows > 0))
        return fail(IHG_ERR_INVALID, "%s: null gradient", what);
    if (!aligned16(d_table)) return fail(IHG_ERR_INVALID, "%s: d_table must be 16-byte aligned", what);
    const bool empty = n_bags == 0 || n_words == 0;
    if (!empty) {
        if (d_query == nullptr || table == nullptr || bag_ptr == nullptr || words == nullptr || word_ptr == nullptr || word_pos == nullptr || w_ih == nullptr ||
            w_hh == nullptr || saved == nullptr)
            return fail(IHG_ERR_INVALID, "%s: null operand", what);
        if (!aligned16(table) || !aligned16(saved)) return fail(IHG_ERR_INVALID, "%s: table and saved must be 16-byte aligned", what);
        if (workspace == nullptr || !aligned16(workspace) || workspace_bytes < gru_workspace_floats(n_words, dim) * 4)
            return fail(IHG_ERR_WORKSPACE, "%s: workspace of %lld bytes, %lld needed (16-byte aligned)", what, (long long)workspace_bytes,
                        (long long)(gru_workspace_floats(n_words, dim) * 4));
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (empty) {
        launch_zero_floats(dw_ih, 3 * static_cast<int64_t>(dim) * dim, s);
        launch_zero_floats(dw_hh, 3 * static_cast<int64_t>(dim) * dim, s);
        launch_zero_floats(db_ih, 3 * dim, s);
        launch_zero_floats(db_hh, 3 * dim, s);
        launch_zero_floats(d_table, n_table_rows * dim, s);
        return check_launch(what);
    }
    const GruWorkspace ws = gru_carve(workspace, n_words, dim);
    const GruBwd a{d_query, ld_dq, {bag_ptr, words, bag_order, n_bags}, w_ih, w_hh, saved, ws.dg, ws.dx};
    const GruWgrad g{table, ld_table, words, saved, ws.dg, n_words, gru_slab_len(n_words), ws.slabs};
    switch (dim) {
        case 32: launch_gru_bwd<32>(a, g, dw_ih, dw_hh, db_ih, db_hh, s); break;
        case 64: launch_gru_bwd<64>(a, g, dw_ih, dw_hh, db_ih, db_hh, s); break;
        case 128: launch_gru_bwd<128>(a, g, dw_ih, dw_hh, db_ih, db_hh, s); break;
        default: launch_gru_bwd<256>(a, g, dw_ih, dw_hh, db_ih, db_hh, s); break;
    }
    if (const int rc = check_launch(what); rc != IHG_OK) return rc;
    // d_table[w] = the sum of dx over the positions of word w, in position order (K7); a word that no query has, row 0 included: a zero row
    return ihg_node_segment_sum(ws.dx, dim, word_ptr, word_pos, nullptr, nullptr, nullptr, nullptr, IHG_SCALE_NONE, d_table, dim, n_table_rows, dim, 0, nullptr, nullptr,
                                0, nullptr, nullptr, 0, nullptr, nullptr, nullptr, stream);
}

}  // extern "C"
