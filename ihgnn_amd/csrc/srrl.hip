// srrl.hip - the kernels of the Srrl baseline (Models/Srrl.py): every module of that model is the block
//     F.normalize(cat(a, b), dim=-1) -> nn.Linear -> optional nn.LeakyReLU()
// over a few hundred to a few thousand rows, so one launch covers what the framework issues as cat / normalize / Linear / LeakyReLU with a [rows, 2d] temporary each.
// Beside the block: the broadcast row dot of the KG scores, the KG loss with its gradient, and a top-k over dense score rows.
// Everything here sums in a fixed order (no float atomics): results are bitwise reproducible.
#include "common.hpp"

namespace {

constexpr int kTileRows = 16;           // rows one workgroup stages at a time
constexpr int kCatMaxWidth = 256;       // widest concatenated row / widest output row of the block kernels (three staged tiles in 64 KiB of LDS)
constexpr int kCatSlabs = 64;           // workgroups (= partial weight gradients) of the backward
constexpr float kNormEps = 1e-12f;      // F.normalize's eps
constexpr float kInvNormEps = 1.0f / kNormEps;
// The backward tells a clamped row (|x| < eps) by its stored inverse norm, which the forward wrote as 1 / max(|x|, eps).  It does not rest on the device's division
// reproducing the compile-time constant bit for bit: anything within 1e-6 of 1 / eps counts as clamped.  So a row whose norm sits in [eps, eps (1 + 1e-6)) is
// treated as clamped, where torch's clamp_min passes the norm's gradient (it passes it at |x| == eps exactly): a sliver of measure ~0 around 1e-12.
constexpr float kClampedInvNorm = kInvNormEps * 0.999999f;
constexpr float kLeakySlope = 0.01f;    // nn.LeakyReLU()'s default

// one operand of the concatenation: row r of the block reads table row idx[r / rep] (idx == nullptr: row r / rep)
struct CatSource {
    const float* base;
    int64_t ld;
    int32_t width;
    const int64_t* idx;
    int64_t rep;
};

__device__ __forceinline__ const float* source_row(const CatSource& s, int64_t r) {
    const int64_t g = r / s.rep;
    return s.base + (s.idx ? s.idx[g] : g) * s.ld;
}

// sum over the 16 lanes that share a staged row (lanes 16 j .. 16 j + 15 of a wave): a fixed butterfly, every lane gets the sum
__device__ __forceinline__ float sum16(float v) {
#pragma unroll
    for (int off = 8; off > 0; off >>= 1) v += __shfl_xor(v, off, 16);
    return v;
}

// stage rows r0 .. r0 + 15 of cat(a, b) into xs (rows beyond n_rows: zeros)
__device__ __forceinline__ void stage_rows(const CatSource& a, const CatSource& b, int64_t r0, int64_t n_rows, float (*xs)[kCatMaxWidth + 1]) {
    const int K = a.width + b.width;
    for (int e = threadIdx.x; e < kTileRows * K; e += kBlockThreads) {
        const int r = e / K, k = e - r * K;
        const int64_t row = r0 + r;
        float v = 0.f;
        if (row < n_rows) v = k < a.width ? source_row(a, row)[k] : source_row(b, row)[k - a.width];
        xs[r][k] = v;
    }
}

__global__ __launch_bounds__(kBlockThreads) void cat_linear_fwd_kernel(CatSource a, CatSource b, const float* __restrict__ w, int64_t ld_w, const float* __restrict__ bias, int m,
                                                                       int normalize, int leaky, float* __restrict__ out, int64_t ld_out, float* __restrict__ inv_norm,
                                                                       int64_t n_rows) {
    __shared__ float xs[kTileRows][kCatMaxWidth + 1];
    __shared__ float inv_s[kTileRows];
    const int K = a.width + b.width;
    const int64_t tiles = (n_rows + kTileRows - 1) / kTileRows;
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t r0 = tile * kTileRows;
        stage_rows(a, b, r0, n_rows, xs);
        __syncthreads();
        {   // the row's 1 / max(|x|, eps): 16 lanes per row
            const int r = threadIdx.x >> 4, l = threadIdx.x & 15;
            float ss = 0.f;
            for (int k = l; k < K; k += 16) ss = fmaf(xs[r][k], xs[r][k], ss);
            ss = sum16(ss);
            const float inv = normalize ? 1.0f / fmaxf(sqrtf(ss), kNormEps) : 1.0f;
            if (l == 0) {
                inv_s[r] = inv;
                if (inv_norm && normalize && r0 + r < n_rows) inv_norm[r0 + r] = inv;
            }
        }
        __syncthreads();
        for (int o = threadIdx.x; o < kTileRows * m; o += kBlockThreads) {
            const int r = o / m, c = o - r * m;
            const int64_t row = r0 + r;
            if (row >= n_rows) continue;
            const float* wr = w + static_cast<int64_t>(c) * ld_w;
            float acc = 0.f;
            for (int k = 0; k < K; ++k) acc = fmaf(wr[k], xs[r][k], acc);
            float v = acc * inv_s[r] + (bias ? bias[c] : 0.f);      // W (x / n) = (W x) / n
            if (leaky) v = v > 0.f ? v : kLeakySlope * v;
            out[row * ld_out + c] = v;
        }
        __syncthreads();
    }
}

// K = 64 / 128 (d = 32 / 64) with 16-byte aligned rows: the same block on the matrix cores, exact fp32 (v_mfma_f32_32x32x2_f32).  A workgroup stages TE rows of
// cat(a, b) in LDS with 16-byte loads, forms the rows' inverse norms there, and its four waves take the (32-row, 32-column) output tiles in turn: the A operand of
// step (t, s) is x[row][8 t + 4 half + s] from LDS, the B operand w[col][8 t + 4 half + s] straight from the weight (at most 64 KiB, cache-resident; 16 bytes per
// lane and t).  Columns beyond m (m = 1: the score head) multiply zeros and are not stored.  The scale and the bias come in the epilogue, as in the any-width kernel.
template <int K>
__global__ __launch_bounds__(kBlockThreads) void cat_linear_fwd_mfma_kernel(CatSource a, CatSource b, const float* __restrict__ w, int64_t ld_w, const float* __restrict__ bias,
                                                                            int m, int normalize, int leaky, float* __restrict__ out, int64_t ld_out,
                                                                            float* __restrict__ inv_norm, int64_t n_rows) {
    constexpr int TE = K == 64 ? 128 : 64, ET = TE / 32, STRIDE = K + kRowPad, V4_PER_ROW = K / 4, T_STEPS = K / 8;
    __shared__ __attribute__((aligned(16))) float xt[TE][STRIDE];
    __shared__ float inv_s[TE];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, l31 = lane & 31;
    const int64_t tiles = (n_rows + TE - 1) / TE;
    const int col_tiles = (m + 31) / 32, jobs = ET * col_tiles, va = a.width / 4;
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t r0 = tile * TE;
        for (int idx = tid; idx < TE * V4_PER_ROW; idx += kBlockThreads) {
            const int r = idx / V4_PER_ROW, v = idx - r * V4_PER_ROW;
            const int64_t row = r0 + r;
            v4f x = {0.f, 0.f, 0.f, 0.f};
            if (row < n_rows) x = *reinterpret_cast<const v4f*>(v < va ? source_row(a, row) + 4 * v : source_row(b, row) + 4 * (v - va));
            *reinterpret_cast<v4f*>(&xt[r][4 * v]) = x;
        }
        __syncthreads();
        for (int r = tid >> 4; r < TE; r += kBlockThreads / 16) {
            const int l = tid & 15;
            float ss = 0.f;
            for (int k = l; k < K; k += 16) ss = fmaf(xt[r][k], xt[r][k], ss);
            ss = sum16(ss);
            const float inv = normalize ? 1.0f / fmaxf(sqrtf(ss), kNormEps) : 1.0f;
            if (l == 0) {
                inv_s[r] = inv;
                if (inv_norm && normalize && r0 + r < n_rows) inv_norm[r0 + r] = inv;
            }
        }
        __syncthreads();
        for (int job = wave; job < jobs; job += kWavesPerBlock) {
            const int et = job % ET, ct = job / ET;
            const int c = ct * 32 + l31;
            const float* wr = w + static_cast<int64_t>(c) * ld_w + 4 * half;
            v16f acc;
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll 4
            for (int t = 0; t < T_STEPS; ++t) {
                const v4f av = *reinterpret_cast<const v4f*>(&xt[et * 32 + l31][8 * t + 4 * half]);
                v4f bv = {0.f, 0.f, 0.f, 0.f};
                if (c < m) bv = *reinterpret_cast<const v4f*>(wr + 8 * t);
#pragma unroll
                for (int s = 0; s < 4; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[s], bv[s], acc, 0, 0, 0);
            }
            if (c < m) {
                const float bias_c = bias ? bias[c] : 0.f;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int tr = et * 32 + acc_row(r, lane);
                    if (r0 + tr >= n_rows) continue;
                    float v = acc[r] * inv_s[tr] + bias_c;
                    if (leaky) v = v > 0.f ? v : kLeakySlope * v;
                    out[(r0 + tr) * ld_out + c] = v;
                }
            }
        }
        __syncthreads();
    }
}

// One workgroup per slab: its tiles' part of dW | dbias goes to slab[blockIdx.x] (assigned on its first tile, added to afterwards - the same thread owns an element
// every time), the rows' input gradients to da / db where rep == 1 and to dx_rows [n_rows, K] (summed over the groups afterwards) where rep > 1.
__global__ __launch_bounds__(kBlockThreads) void cat_linear_bwd_kernel(CatSource a, CatSource b, const float* __restrict__ dy, int64_t ld_dy, const float* __restrict__ y, int64_t ld_y,
                                                                       const float* __restrict__ inv_norm, const float* __restrict__ w, int64_t ld_w, int m, int normalize,
                                                                       int leaky, float* __restrict__ slabs, float* __restrict__ da, int64_t ld_da, float* __restrict__ db,
                                                                       int64_t ld_db, float* __restrict__ dx_rows, int64_t n_rows) {
    __shared__ float xs[kTileRows][kCatMaxWidth + 1];      // the Linear's input: x / max(|x|, eps), or x
    __shared__ float dxs[kTileRows][kCatMaxWidth + 1];     // its gradient
    __shared__ float dps[kTileRows][kCatMaxWidth + 1];     // dy * act'(y)
    __shared__ float inv_s[kTileRows], dot_s[kTileRows];
    const int K = a.width + b.width;
    const int64_t tiles = (n_rows + kTileRows - 1) / kTileRows;
    float* slab = slabs + static_cast<int64_t>(blockIdx.x) * (static_cast<int64_t>(m) * K + m);
    bool first = true;
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t r0 = tile * kTileRows;
        stage_rows(a, b, r0, n_rows, xs);
        if (threadIdx.x < kTileRows) inv_s[threadIdx.x] = (normalize && r0 + threadIdx.x < n_rows) ? inv_norm[r0 + threadIdx.x] : 1.0f;
        for (int e = threadIdx.x; e < kTileRows * m; e += kBlockThreads) {
            const int r = e / m, c = e - r * m;
            const int64_t row = r0 + r;
            float v = 0.f;
            if (row < n_rows) {
                v = dy[row * ld_dy + c];
                if (leaky && !(y[row * ld_y + c] > 0.f)) v *= kLeakySlope;
            }
            dps[r][c] = v;
        }
        __syncthreads();
        for (int e = threadIdx.x; e < kTileRows * K; e += kBlockThreads) {
            const int r = e / K, k = e - r * K;
            xs[r][k] *= inv_s[r];
        }
        __syncthreads();
        // dW[c][k] += sum_r dps[r][c] xs[r][k], dbias[c] += sum_r dps[r][c]: rows in ascending order
        const int n_w = m * K;
        for (int e = threadIdx.x; e < n_w + m; e += kBlockThreads) {
            float s = 0.f;
            if (e < n_w) {
                const int c = e / K, k = e - c * K;
#pragma unroll
                for (int r = 0; r < kTileRows; ++r) s = fmaf(dps[r][c], xs[r][k], s);
            } else {
                const int c = e - n_w;
#pragma unroll
                for (int r = 0; r < kTileRows; ++r) s += dps[r][c];
            }
            slab[e] = first ? s : slab[e] + s;
        }
        first = false;
        if (da || db) {
            for (int e = threadIdx.x; e < kTileRows * K; e += kBlockThreads) {
                const int r = e / K, k = e - r * K;
                float s = 0.f;
                for (int c = 0; c < m; ++c) s = fmaf(dps[r][c], w[static_cast<int64_t>(c) * ld_w + k], s);
                dxs[r][k] = s;
            }
            __syncthreads();
            if (normalize) {
                const int r = threadIdx.x >> 4, l = threadIdx.x & 15;
                float dot = 0.f;
                for (int k = l; k < K; k += 16) dot = fmaf(xs[r][k], dxs[r][k], dot);
                dot = sum16(dot);
                if (l == 0) dot_s[r] = dot;
                __syncthreads();
            }
            for (int e = threadIdx.x; e < kTileRows * K; e += kBlockThreads) {
                const int r = e / K, k = e - r * K;
                const int64_t row = r0 + r;
                if (row >= n_rows) continue;
                float v = dxs[r][k];
                if (normalize) {
                    const float inv = inv_s[r];
                    // autograd of x / clamp_min(|x|, eps): the clamp passes no gradient to the norm below eps
                    v = inv < kClampedInvNorm ? (v - xs[r][k] * dot_s[r]) * inv : v * kInvNormEps;
                }
                if (k < a.width) {
                    if (da) (a.rep == 1 ? da + row * ld_da : dx_rows + row * K)[k] = v;
                } else if (db) {
                    if (b.rep == 1) db[row * ld_db + (k - a.width)] = v;
                    else dx_rows[row * K + k] = v;
                }
            }
        }
        __syncthreads();
    }
}

// The backward at K = 64 / 128 with m <= 128 and 16-byte aligned source rows: the same slabs, row gradients and workspace as cat_linear_bwd_kernel, with the two
// contractions on the matrix cores (fp32 MFMA, exact).  32 rows per trip: dW's tiles (32 outputs x 32 columns) contract the trip's 32 rows, A = dz[row][c] and
// B = x^[row][k] both read down the staged tiles; dx^'s tiles (32 rows x 32 columns) contract the outputs, A = dz[row][8 t + 4 half + s] and B = w[c][k] from the
// weight.  Outputs beyond m are zeros in dz.  A wave keeps its tiles from trip to trip, so the same lane owns a slab element every time.
template <int K>
__global__ __launch_bounds__(kBlockThreads) void cat_linear_bwd_mfma_kernel(CatSource a, CatSource b, const float* __restrict__ dy, int64_t ld_dy, const float* __restrict__ y,
                                                                            int64_t ld_y, const float* __restrict__ inv_norm, const float* __restrict__ w, int64_t ld_w, int m,
                                                                            int normalize, int leaky, float* __restrict__ slabs, float* __restrict__ da, int64_t ld_da,
                                                                            float* __restrict__ db, int64_t ld_db, float* __restrict__ dx_rows, int64_t n_rows) {
    constexpr int TE = 32, STRIDE = K + kRowPad, MSTRIDE = 128 + kRowPad, V4_PER_ROW = K / 4, KT = K / 32;
    __shared__ __attribute__((aligned(16))) float xt[TE][STRIDE];       // x^ (or x)
    __shared__ __attribute__((aligned(16))) float dxt[TE][STRIDE];      // its gradient
    __shared__ __attribute__((aligned(16))) float dzt[TE][MSTRIDE];     // dy * act'(y), zeros beyond m
    __shared__ float inv_s[TE], dot_s[TE];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, l31 = lane & 31;
    const int m_pad = (m + 31) & ~31, va = a.width / 4;
    const int64_t tiles = (n_rows + TE - 1) / TE;
    float* slab = slabs + static_cast<int64_t>(blockIdx.x) * (static_cast<int64_t>(m) * K + m);
    bool first = true;
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t r0 = tile * TE;
        if (tid < TE) inv_s[tid] = (normalize && r0 + tid < n_rows) ? inv_norm[r0 + tid] : 1.0f;
        __syncthreads();
        for (int idx = tid; idx < TE * V4_PER_ROW; idx += kBlockThreads) {
            const int r = idx / V4_PER_ROW, v = idx - r * V4_PER_ROW;
            const int64_t row = r0 + r;
            v4f x = {0.f, 0.f, 0.f, 0.f};
            if (row < n_rows) x = *reinterpret_cast<const v4f*>(v < va ? source_row(a, row) + 4 * v : source_row(b, row) + 4 * (v - va));
            *reinterpret_cast<v4f*>(&xt[r][4 * v]) = x * inv_s[r];
        }
        for (int e = tid; e < TE * m_pad; e += kBlockThreads) {
            const int r = e / m_pad, c = e - r * m_pad;
            const int64_t row = r0 + r;
            float v = 0.f;
            if (row < n_rows && c < m) {
                v = dy[row * ld_dy + c];
                if (leaky && !(y[row * ld_y + c] > 0.f)) v *= kLeakySlope;
            }
            dzt[r][c] = v;
        }
        __syncthreads();
        // dW tiles
        for (int job = wave; job < (m_pad / 32) * KT; job += kWavesPerBlock) {
            const int jt = job / KT, kt = job - jt * KT;
            v16f acc;
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll 4
            for (int e2 = 0; e2 < TE / 2; ++e2) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(dzt[2 * e2 + half][jt * 32 + l31], xt[2 * e2 + half][kt * 32 + l31], acc, 0, 0, 0);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int c = jt * 32 + acc_row(r, lane);
                if (c < m) {
                    float* p = slab + static_cast<int64_t>(c) * K + kt * 32 + l31;
                    *p = first ? acc[r] : *p + acc[r];
                }
            }
        }
        if (tid < m) {
            float s = 0.f;
#pragma unroll 8
            for (int r = 0; r < TE; ++r) s += dzt[r][tid];
            float* p = slab + static_cast<int64_t>(m) * K + tid;
            *p = first ? s : *p + s;
        }
        first = false;
        if (da || db) {
            for (int kt = wave; kt < KT; kt += kWavesPerBlock) {
                v16f acc;
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[r] = 0.f;
                for (int t = 0; t < m_pad / 8; ++t) {
                    const v4f av = *reinterpret_cast<const v4f*>(&dzt[l31][8 * t + 4 * half]);
#pragma unroll
                    for (int s = 0; s < 4; ++s) {
                        const int c = 8 * t + 4 * half + s;
                        const float bv = c < m ? w[static_cast<int64_t>(c) * ld_w + kt * 32 + l31] : 0.f;
                        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[s], bv, acc, 0, 0, 0);
                    }
                }
#pragma unroll
                for (int r = 0; r < 16; ++r) dxt[acc_row(r, lane)][kt * 32 + l31] = acc[r];
            }
            __syncthreads();
            if (normalize) {
                for (int r = tid >> 4; r < TE; r += kBlockThreads / 16) {
                    const int l = tid & 15;
                    float dot = 0.f;
                    for (int k = l; k < K; k += 16) dot = fmaf(xt[r][k], dxt[r][k], dot);
                    dot = sum16(dot);
                    if (l == 0) dot_s[r] = dot;
                }
                __syncthreads();
            }
            for (int e = tid; e < TE * K; e += kBlockThreads) {
                const int r = e / K, k = e - r * K;
                const int64_t row = r0 + r;
                if (row >= n_rows) continue;
                float v = dxt[r][k];
                if (normalize) {
                    const float inv = inv_s[r];
                    v = inv < kClampedInvNorm ? (v - xt[r][k] * dot_s[r]) * inv : v * kInvNormEps;
                }
                if (k < a.width) {
                    if (da) (a.rep == 1 ? da + row * ld_da : dx_rows + row * K)[k] = v;
                } else if (db) {
                    if (b.rep == 1) db[row * ld_db + (k - a.width)] = v;
                    else dx_rows[row * K + k] = v;
                }
            }
        }
        __syncthreads();
    }
}

// out[g][c] = sum_{j < rep} rows[(g rep + j) ld + c], j ascending
__global__ __launch_bounds__(kBlockThreads) void group_sum_kernel(const float* __restrict__ rows, int64_t ld, int64_t rep, int width, float* __restrict__ out, int64_t ld_out,
                                                                  int64_t n_groups) {
    const int64_t total = n_groups * width;
    for (int64_t e = static_cast<int64_t>(blockIdx.x) * kBlockThreads + threadIdx.x; e < total; e += static_cast<int64_t>(gridDim.x) * kBlockThreads) {
        const int64_t g = e / width;
        const int c = static_cast<int>(e - g * width);
        const float* p = rows + g * rep * ld + c;
        float s = 0.f;
        for (int64_t j = 0; j < rep; ++j) s += p[j * ld];
        out[g * ld_out + c] = s;
    }
}

// dW | dbias = the slabs added in slab order (slab_sum's fixed tree)
__global__ __launch_bounds__(kBlockThreads) void cat_linear_slab_kernel(const float* __restrict__ slabs, int n_slabs, int m, int K, float* __restrict__ dw, int64_t ld_dw,
                                                                        float* __restrict__ dbias) {
    const int64_t total = static_cast<int64_t>(m) * K + m;
    const int64_t idx = static_cast<int64_t>(blockIdx.x) * kWave + (threadIdx.x & 63);
    const bool live = idx < total;
    const float sum = slab_sum(slabs, n_slabs, total, idx, live);
    if (threadIdx.x < kWave && live) {
        if (idx < static_cast<int64_t>(m) * K) {
            dw[(idx / K) * ld_dw + idx % K] = sum;
        } else if (dbias) {
            dbias[idx - static_cast<int64_t>(m) * K] = sum;
        }
    }
}

__global__ __launch_bounds__(kBlockThreads) void rows_dot_fwd_kernel(const float* __restrict__ x, int64_t ld_x, const float* __restrict__ y, int64_t ld_y, int64_t rep,
                                                                     float* __restrict__ s, int64_t n_rows, int width) {
    for (int64_t r = static_cast<int64_t>(blockIdx.x) * kBlockThreads + threadIdx.x; r < n_rows; r += static_cast<int64_t>(gridDim.x) * kBlockThreads) {
        const float* xr = x + r * ld_x;
        const float* yr = y + (r / rep) * ld_y;
        float acc = 0.f;
        for (int c = 0; c < width; ++c) acc = fmaf(xr[c], yr[c], acc);
        s[r] = acc;
    }
}

__global__ __launch_bounds__(kBlockThreads) void rows_dot_bwd_x_kernel(const float* __restrict__ ds, const float* __restrict__ y, int64_t ld_y, int64_t rep, float* __restrict__ dx,
                                                                       int64_t ld_dx, int64_t n_rows, int width) {
    const int64_t total = n_rows * width;
    for (int64_t e = static_cast<int64_t>(blockIdx.x) * kBlockThreads + threadIdx.x; e < total; e += static_cast<int64_t>(gridDim.x) * kBlockThreads) {
        const int64_t r = e / width;
        const int c = static_cast<int>(e - r * width);
        dx[r * ld_dx + c] = ds[r] * y[(r / rep) * ld_y + c];
    }
}

__global__ __launch_bounds__(kBlockThreads) void rows_dot_bwd_y_kernel(const float* __restrict__ ds, const float* __restrict__ x, int64_t ld_x, int64_t rep, float* __restrict__ dy,
                                                                       int64_t ld_dy, int64_t n_groups, int width) {
    const int64_t total = n_groups * width;
    for (int64_t e = static_cast<int64_t>(blockIdx.x) * kBlockThreads + threadIdx.x; e < total; e += static_cast<int64_t>(gridDim.x) * kBlockThreads) {
        const int64_t g = e / width;
        const int c = static_cast<int>(e - g * width);
        float acc = 0.f;
        for (int64_t j = 0; j < rep; ++j) acc = fmaf(ds[g * rep + j], x[(g * rep + j) * ld_x + c], acc);
        dy[g * ld_dy + c] = acc;
    }
}

// sum over the workgroup in a fixed order: lanes by butterfly, then the four waves in wave order; every thread gets the sum
__device__ __forceinline__ float block_sum(float v, float* part) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
    __syncthreads();
    return (part[0] + part[1]) + (part[2] + part[3]);
}

__device__ __forceinline__ float log_sigmoid(float x) { return fminf(x, 0.f) - log1pf(expf(-fabsf(x))); }
__device__ __forceinline__ float sigmoid(float x) {
    const float e = expf(-fabsf(x));
    return x >= 0.f ? 1.0f / (1.0f + e) : e / (1.0f + e);
}

// one workgroup: the batch is a few hundred rows
__global__ __launch_bounds__(kBlockThreads) void kg_loss_kernel(const float* __restrict__ pos, const float* __restrict__ neg, int64_t ld_neg, const float* __restrict__ weight,
                                                                int64_t B, int k, float* __restrict__ loss, float* __restrict__ dpos, float* __restrict__ dneg, int64_t ld_dneg) {
    __shared__ float part[kWavesPerBlock];
    float ws = 0.f;
    for (int64_t r = threadIdx.x; r < B; r += kBlockThreads) ws += weight ? weight[r] : 1.0f;
    const float wsum = block_sum(ws, part);
    float lp = 0.f, ln = 0.f;
    for (int64_t r = threadIdx.x; r < B; r += kBlockThreads) {
        const float wr = weight ? weight[r] : 1.0f;
        const float p = pos[r];
        lp = fmaf(wr, log_sigmoid(p), lp);
        dpos[r] = -0.5f * (wr / wsum) * sigmoid(-p);
        float s = 0.f;
        const float gscale = 0.5f * (wr / wsum) / static_cast<float>(k);
        for (int j = 0; j < k; ++j) {
            const float n = neg[r * ld_neg + j];
            s += log_sigmoid(-n);
            dneg[r * ld_dneg + j] = gscale * sigmoid(n);
        }
        ln = fmaf(wr, s / static_cast<float>(k), ln);
    }
    const float lp_sum = block_sum(lp, part);
    const float ln_sum = block_sum(ln, part);
    if (threadIdx.x == 0) loss[0] = 0.5f * (-(lp_sum / wsum) - (ln_sum / wsum));
}

struct Best {
    float s;
    int64_t i;      // -1: none
};
// the ranking order: higher score first, equal scores in ascending item id
__device__ __forceinline__ bool better(const Best& p, const Best& q) {
    if (p.i < 0) return false;
    if (q.i < 0) return true;
    return p.s > q.s || (p.s == q.s && p.i < q.i);
}

// one workgroup per score row; pass j finds the best entry that ranks behind the one pass j - 1 found (a total order: no entry is found twice, ties included)
__global__ __launch_bounds__(kBlockThreads) void rows_topk_kernel(const float* __restrict__ scores, int64_t ld, int64_t n_items, int k, int64_t* __restrict__ out_items,
                                                                  float* __restrict__ out_scores, int64_t n_rows) {
    __shared__ float best_s[kWavesPerBlock];
    __shared__ int64_t best_i[kWavesPerBlock];
    for (int64_t row = blockIdx.x; row < n_rows; row += gridDim.x) {
        const float* sr = scores + row * ld;
        Best prev{0.f, -1};
        bool done = false;
        for (int j = 0; j < k; ++j) {
            Best mine{0.f, -1};
            if (!done) {
                for (int64_t i = threadIdx.x; i < n_items; i += kBlockThreads) {
                    const float s = sr[i];
                    if (s != s) continue;                                          // a NaN is never ranked
                    if (prev.i >= 0 && !(s < prev.s || (s == prev.s && i > prev.i))) continue;
                    const Best cand{s, i};
                    if (better(cand, mine)) mine = cand;
                }
#pragma unroll
                for (int off = 32; off > 0; off >>= 1) {
                    Best other;
                    other.s = __shfl_xor(mine.s, off, 64);
                    const int lo = __shfl_xor(static_cast<int>(mine.i & 0xffffffff), off, 64), hi = __shfl_xor(static_cast<int>(mine.i >> 32), off, 64);
                    other.i = (static_cast<int64_t>(hi) << 32) | static_cast<uint32_t>(lo);
                    if (better(other, mine)) mine = other;
                }
                if ((threadIdx.x & 63) == 0) {
                    best_s[threadIdx.x >> 6] = mine.s;
                    best_i[threadIdx.x >> 6] = mine.i;
                }
            }
            __syncthreads();
            if (!done) {
                mine = Best{best_s[0], best_i[0]};
#pragma unroll
                for (int wv = 1; wv < kWavesPerBlock; ++wv) {
                    const Best other{best_s[wv], best_i[wv]};
                    if (better(other, mine)) mine = other;
                }
                if (mine.i < 0) done = true;
                prev = mine;
            }
            if (threadIdx.x == 0) {
                out_items[row * k + j] = done ? -1 : prev.i;
                out_scores[row * k + j] = done ? -INFINITY : prev.s;
            }
            __syncthreads();
        }
    }
}

inline int grid_for_elements(int64_t n) {
    return static_cast<int>(std::max<int64_t>(1, std::min<int64_t>((n + kBlockThreads - 1) / kBlockThreads, kMaxBlocks)));
}

// the shared front of the two block entry points
int check_block(const char* name, const float* a, int64_t ld_a, int32_t width_a, int64_t rep_a, const float* b, int64_t ld_b, int32_t width_b, int64_t rep_b, const float* w,
                int64_t ld_w, int32_t m, int32_t activation, int64_t n_rows) {
    if (width_a <= 0 || width_b < 0 || m <= 0 || n_rows < 0 || rep_a < 1 || rep_b < 1)
        return fail(IHG_ERR_INVALID, "%s: bad size (widths %d + %d, m %d, %lld rows, rep %lld / %lld)", name, width_a, width_b, m, (long long)n_rows, (long long)rep_a, (long long)rep_b);
    const int K = width_a + width_b;
    if (K > kCatMaxWidth || m > kCatMaxWidth) return fail(IHG_ERR_INVALID, "%s: width %d -> %d beyond %d", name, K, m, kCatMaxWidth);
    if (ld_a < width_a || (width_b > 0 && ld_b < width_b) || ld_w < K) return fail(IHG_ERR_INVALID, "%s: bad leading dimension", name);
    if (activation != IHG_ACT_NONE && activation != IHG_ACT_LEAKY_RELU) return fail(IHG_ERR_INVALID, "%s: activation %d", name, activation);
    if (n_rows % rep_a != 0 || n_rows % rep_b != 0) return fail(IHG_ERR_INVALID, "%s: %lld rows are not whole groups of %lld / %lld", name, (long long)n_rows, (long long)rep_a, (long long)rep_b);
    (void)a; (void)b; (void)w;
    return IHG_OK;
}

constexpr int kCatMfmaBlocks = 1024;      // workgroups of the matrix-core forward (four fit a CU's LDS): one trip each up to 131072 rows at K = 64, 65536 at K = 128

// K = 64 / 128 with every row of both sources and of the weight on a 16-byte boundary
inline bool cat_linear_on_matrix_cores(const float* a, int64_t ld_a, int32_t width_a, const float* b, int64_t ld_b, int32_t width_b, const float* w, int64_t ld_w) {
    const int K = width_a + width_b;
    if (K != 64 && K != 128) return false;
    if (width_a % 4 != 0 || !aligned16(a) || ld_a % 4 != 0 || !aligned16(w) || ld_w % 4 != 0) return false;
    return width_b == 0 || (aligned16(b) && ld_b % 4 == 0);
}

}  // namespace

extern "C" {

int32_t ihg_cat_linear_max_width(void) { return kCatMaxWidth; }

int64_t ihg_cat_linear_workspace_bytes(int64_t n_rows, int32_t width, int32_t m) {
    if (n_rows < 0 || width <= 0 || m <= 0 || width > kCatMaxWidth || m > kCatMaxWidth) return -1;
    return 4 * (static_cast<int64_t>(kCatSlabs) * (static_cast<int64_t>(m) * width + m) + n_rows * width);
}

int ihg_cat_linear_fwd(const float* a, int64_t ld_a, int32_t width_a, const int64_t* idx_a, int64_t rep_a, const float* b, int64_t ld_b, int32_t width_b, const int64_t* idx_b,
                       int64_t rep_b, const float* w, int64_t ld_w, const float* bias, int32_t m, int32_t normalize, int32_t activation, float* out, int64_t ld_out,
                       float* inv_norm, int64_t n_rows, ihg_stream_t stream) {
    const char* name = "ihg_cat_linear_fwd";
    if (int rc = check_block(name, a, ld_a, width_a, rep_a, b, ld_b, width_b, rep_b, w, ld_w, m, activation, n_rows)) return rc;
    if (ld_out < m) return fail(IHG_ERR_INVALID, "%s: bad leading dimension", name);
    if (n_rows == 0) return IHG_OK;
    if (!a || (width_b > 0 && !b) || !w || !out || (normalize && !inv_norm)) return fail(IHG_ERR_INVALID, "%s: null pointer", name);
    const CatSource sa{a, ld_a, width_a, idx_a, rep_a}, sb{b, ld_b, width_b, idx_b, rep_b};
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int K = width_a + width_b;
    if (cat_linear_on_matrix_cores(a, ld_a, width_a, b, ld_b, width_b, w, ld_w)) {
        const int64_t tiles = (n_rows + (K == 64 ? 128 : 64) - 1) / (K == 64 ? 128 : 64);
        const int grid = static_cast<int>(std::min<int64_t>(tiles, kCatMfmaBlocks));
        if (K == 64)
            hipLaunchKernelGGL(cat_linear_fwd_mfma_kernel<64>, dim3(grid), dim3(kBlockThreads), 0, s, sa, sb, w, ld_w, bias, m, normalize != 0, activation == IHG_ACT_LEAKY_RELU, out,
                               ld_out, inv_norm, n_rows);
        else
            hipLaunchKernelGGL(cat_linear_fwd_mfma_kernel<128>, dim3(grid), dim3(kBlockThreads), 0, s, sa, sb, w, ld_w, bias, m, normalize != 0, activation == IHG_ACT_LEAKY_RELU, out,
                               ld_out, inv_norm, n_rows);
        return check_launch(name);
    }
    const int64_t tiles = (n_rows + kTileRows - 1) / kTileRows;
    const int grid = static_cast<int>(std::min<int64_t>(tiles, kMaxBlocks));
    hipLaunchKernelGGL(cat_linear_fwd_kernel, dim3(grid), dim3(kBlockThreads), 0, static_cast<hipStream_t>(stream), sa, sb, w, ld_w, bias, m, normalize != 0,
                       activation == IHG_ACT_LEAKY_RELU, out, ld_out, inv_norm, n_rows);
    return check_launch(name);
}

int ihg_cat_linear_bwd(const float* dy, int64_t ld_dy, const float* y, int64_t ld_y, const float* a, int64_t ld_a, int32_t width_a, const int64_t* idx_a, int64_t rep_a,
                       const float* b, int64_t ld_b, int32_t width_b, const int64_t* idx_b, int64_t rep_b, const float* inv_norm, const float* w, int64_t ld_w, int32_t m,
                       int32_t normalize, int32_t activation, float* dw, int64_t ld_dw, float* dbias, float* da, int64_t ld_da, float* db, int64_t ld_db, int64_t n_rows,
                       void* workspace, int64_t workspace_bytes, ihg_stream_t stream) {
    const char* name = "ihg_cat_linear_bwd";
    if (int rc = check_block(name, a, ld_a, width_a, rep_a, b, ld_b, width_b, rep_b, w, ld_w, m, activation, n_rows)) return rc;
    const int K = width_a + width_b;
    if (ld_dy < m || ld_y < m || ld_dw < K || (da && ld_da < width_a) || (db && ld_db < width_b)) return fail(IHG_ERR_INVALID, "%s: bad leading dimension", name);
    if (!dw) return fail(IHG_ERR_INVALID, "%s: null pointer", name);
    if (db && width_b == 0) return fail(IHG_ERR_INVALID, "%s: db without a second source", name);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (n_rows == 0) {      // no rows: zero gradients
        if (ld_dw == K) launch_zero_floats(dw, static_cast<int64_t>(m) * K, s);
        else for (int c = 0; c < m; ++c) launch_zero_floats(dw + c * ld_dw, K, s);
        launch_zero_floats(dbias, dbias ? m : 0, s);
        return check_launch(name);
    }
    if (!dy || !a || (width_b > 0 && !b) || !w || (normalize && !inv_norm) || (activation != IHG_ACT_NONE && !y)) return fail(IHG_ERR_INVALID, "%s: null pointer", name);
    if (!workspace || !aligned16(workspace)) return fail(IHG_ERR_INVALID, "%s: workspace null or not 16-byte aligned", name);
    if (workspace_bytes < ihg_cat_linear_workspace_bytes(n_rows, K, m)) return fail(IHG_ERR_WORKSPACE, "%s: workspace too small", name);
    float* slabs = static_cast<float*>(workspace);
    float* dx_rows = slabs + static_cast<int64_t>(kCatSlabs) * (static_cast<int64_t>(m) * K + m);
    const CatSource sa{a, ld_a, width_a, idx_a, rep_a}, sb{b, ld_b, width_b, idx_b, rep_b};
    const bool matrix_cores = m <= 128 && cat_linear_on_matrix_cores(a, ld_a, width_a, b, ld_b, width_b, w, ld_w);
    const int tile_rows = matrix_cores ? 32 : kTileRows;
    const int64_t tiles = (n_rows + tile_rows - 1) / tile_rows;
    const int n_slabs = static_cast<int>(std::min<int64_t>(tiles, kCatSlabs));
    const bool leaky = activation == IHG_ACT_LEAKY_RELU;
    if (matrix_cores && K == 64)
        hipLaunchKernelGGL(cat_linear_bwd_mfma_kernel<64>, dim3(n_slabs), dim3(kBlockThreads), 0, s, sa, sb, dy, ld_dy, y, ld_y, inv_norm, w, ld_w, m, normalize != 0, leaky, slabs, da,
                           ld_da, db, ld_db, dx_rows, n_rows);
    else if (matrix_cores)
        hipLaunchKernelGGL(cat_linear_bwd_mfma_kernel<128>, dim3(n_slabs), dim3(kBlockThreads), 0, s, sa, sb, dy, ld_dy, y, ld_y, inv_norm, w, ld_w, m, normalize != 0, leaky, slabs, da,
                           ld_da, db, ld_db, dx_rows, n_rows);
    else
        hipLaunchKernelGGL(cat_linear_bwd_kernel, dim3(n_slabs), dim3(kBlockThreads), 0, s, sa, sb, dy, ld_dy, y, ld_y, inv_norm, w, ld_w, m, normalize != 0, leaky, slabs, da, ld_da,
                           db, ld_db, dx_rows, n_rows);
    if (da && rep_a > 1)
        hipLaunchKernelGGL(group_sum_kernel, dim3(grid_for_elements(n_rows / rep_a * width_a)), dim3(kBlockThreads), 0, s, dx_rows, static_cast<int64_t>(K), rep_a, width_a, da, ld_da,
                           n_rows / rep_a);
    if (db && rep_b > 1)
        hipLaunchKernelGGL(group_sum_kernel, dim3(grid_for_elements(n_rows / rep_b * width_b)), dim3(kBlockThreads), 0, s, dx_rows + width_a, static_cast<int64_t>(K), rep_b, width_b, db,
                           ld_db, n_rows / rep_b);
    const int64_t total = static_cast<int64_t>(m) * K + m;
    hipLaunchKernelGGL(cat_linear_slab_kernel, dim3(static_cast<int>((total + kWave - 1) / kWave)), dim3(kBlockThreads), 0, s, slabs, n_slabs, m, K, dw, ld_dw, dbias);
    return check_launch(name);
}

int ihg_rows_dot_fwd(const float* x, int64_t ld_x, const float* y, int64_t ld_y, int64_t rep, float* s, int64_t n_rows, int32_t width, ihg_stream_t stream) {
    const char* name = "ihg_rows_dot_fwd";
    if (width <= 0 || n_rows < 0 || rep < 1 || ld_x < width || ld_y < width || n_rows % rep != 0)
        return fail(IHG_ERR_INVALID, "%s: bad size (%lld rows, width %d, rep %lld)", name, (long long)n_rows, width, (long long)rep);
    if (n_rows == 0) return IHG_OK;
    if (!x || !y || !s) return fail(IHG_ERR_INVALID, "%s: null pointer", name);
    hipLaunchKernelGGL(rows_dot_fwd_kernel, dim3(grid_for_elements(n_rows)), dim3(kBlockThreads), 0, static_cast<hipStream_t>(stream), x, ld_x, y, ld_y, rep, s, n_rows, width);
    return check_launch(name);
}

int ihg_rows_dot_bwd(const float* ds, const float* x, int64_t ld_x, const float* y, int64_t ld_y, int64_t rep, float* dx, int64_t ld_dx, float* dy, int64_t ld_dy, int64_t n_rows,
                     int32_t width, ihg_stream_t stream) {
    const char* name = "ihg_rows_dot_bwd";
    if (width <= 0 || n_rows < 0 || rep < 1 || ld_x < width || ld_y < width || n_rows % rep != 0 || (dx && ld_dx < width) || (dy && ld_dy < width))
        return fail(IHG_ERR_INVALID, "%s: bad size (%lld rows, width %d, rep %lld)", name, (long long)n_rows, width, (long long)rep);
    if (n_rows == 0) return IHG_OK;
    if (!ds || !x || !y) return fail(IHG_ERR_INVALID, "%s: null pointer", name);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (dx) hipLaunchKernelGGL(rows_dot_bwd_x_kernel, dim3(grid_for_elements(n_rows * width)), dim3(kBlockThreads), 0, s, ds, y, ld_y, rep, dx, ld_dx, n_rows, width);
    if (dy) hipLaunchKernelGGL(rows_dot_bwd_y_kernel, dim3(grid_for_elements(n_rows / rep * width)), dim3(kBlockThreads), 0, s, ds, x, ld_x, rep, dy, ld_dy, n_rows / rep, width);
    return check_launch(name);
}

int ihg_kg_loss(const float* pos, const float* neg, int64_t ld_neg, const float* weight, int64_t batch, int32_t k, float* loss, float* dpos, float* dneg, int64_t ld_dneg,
                ihg_stream_t stream) {
    const char* name = "ihg_kg_loss";
    if (batch < 1 || batch > (1 << 24) || k < 1 || ld_neg < k || ld_dneg < k) return fail(IHG_ERR_INVALID, "%s: bad size (batch %lld, k %d)", name, (long long)batch, k);
    if (!pos || !neg || !loss || !dpos || !dneg) return fail(IHG_ERR_INVALID, "%s: null pointer", name);
    hipLaunchKernelGGL(kg_loss_kernel, dim3(1), dim3(kBlockThreads), 0, static_cast<hipStream_t>(stream), pos, neg, ld_neg, weight, batch, k, loss, dpos, dneg, ld_dneg);
    return check_launch(name);
}

int ihg_rows_topk(const float* scores, int64_t ld, int64_t n_rows, int64_t n_items, int32_t k, int64_t* items, float* top_scores, ihg_stream_t stream) {
    const char* name = "ihg_rows_topk";
    if (k < 1 || k > 128) return fail(IHG_ERR_INVALID, "%s: k %d outside 1 .. 128", name, k);
    if (n_rows < 0 || n_items < 0 || ld < n_items) return fail(IHG_ERR_INVALID, "%s: bad size (%lld rows of %lld items, ld %lld)", name, (long long)n_rows, (long long)n_items, (long long)ld);
    if (n_rows == 0) return IHG_OK;
    if ((n_items > 0 && !scores) || !items || !top_scores) return fail(IHG_ERR_INVALID, "%s: null pointer", name);
    const int grid = static_cast<int>(std::min<int64_t>(n_rows, kMaxBlocks));
    hipLaunchKernelGGL(rows_topk_kernel, dim3(grid), dim3(kBlockThreads), 0, static_cast<hipStream_t>(stream), scores, ld, n_items, k, items, top_scores, n_rows);
    return check_launch(name);
}

}  // extern "C"
