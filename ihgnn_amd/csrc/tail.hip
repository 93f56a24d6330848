// tail.hip - the batch tail: HEM scores straight from the layer outputs, BCE-with-logits, per-row gradients and the
// deterministic sort-free scatter of duplicate rows.
#include "common.hpp"

namespace {

// ================================================================================================
// Batch tail (HEM scoring head over the concatenated layer outputs, Models/PredictionLayers.py:21-44 after
// Models/RawGnn.py:122-131): one wave per batch row, lanes over the columns of every layer output; no [N, D] concat.
//   fwd  score[r] = sum_l sum_c X_l[item_r][c] * (lam * X_l[query_r][c] + (1 - lam) * X_l[user_r][c]) + bias[item_r]
//   bwd  rowgrad[0B + r] = ds (1 - lam) X[item_r]   (w.r.t. the user row),   rowgrad[1B + r] = ds lam X[item_r]   (query row),
//        rowgrad[2B + r] = ds (lam X[query_r] + (1 - lam) X[user_r])   (item row); [3B, L1*d] dense and conflict-free -
//        the caller adds duplicate rows with one deterministic scatter.
// ================================================================================================
// per layer: the matrix (virtual base, common.hpp TypedRows) its user / query / item rows are read from - three equal pointers for an ordinary [N, d] layer
// output; layer 0 may be the embedding tables themselves (rows 1.. of the user table, the queries' bag means, rows 1.. of the item table): a batch's user,
// query and item rows are typed by construction, so the head needs no type lookup
struct LayerPtrs {
    const float* x[8][3];
    int64_t ld[8];
};

// rows_upper (optional): the rows of the layers ABOVE layer 0 where they are numbered differently from layer 0's - a layout that leaves the isolated nodes out of its own
// numbering (IncidenceLayout.node_map) while layer 0 is read from the embedding tables by public id; a negative entry is an isolated node: its rows above layer 0 are zero
// (constants: the row gradients written for them are never added anywhere - ihg_batch_rows_add / _put skip negative rows)
struct BatchRow {
    const float *pu, *pq, *pi;                              // the user / query / item row of batch row r in layer l (the layer's first row where the id is negative: not read)
    int64_t u, q, it;                                       // their ids; negative = a zero row
};

__device__ __forceinline__ BatchRow batch_row(const LayerPtrs& layers, int l, const int64_t* __restrict__ rows, const int64_t* __restrict__ rows_upper, int64_t batch, int64_t r) {
    const int64_t* rr = (l > 0 && rows_upper != nullptr) ? rows_upper : rows;
    const int64_t u = rr[r], q = rr[batch + r], it = rr[2 * batch + r];
    return {layers.x[l][0] + (u < 0 ? 0 : u) * layers.ld[l], layers.x[l][1] + (q < 0 ? 0 : q) * layers.ld[l], layers.x[l][2] + (it < 0 ? 0 : it) * layers.ld[l], u, q, it};
}

// optional extra column of the row gradients (width > L1 * d): d bias, carried by the item row
__device__ __forceinline__ void bias_column(float* __restrict__ rowgrad, int64_t width, int n_layers, int dim, int64_t batch, int64_t r, float ds) {
    if ((threadIdx.x & 63) == 0 && width > static_cast<int64_t>(n_layers) * dim) {
        const int64_t col = static_cast<int64_t>(n_layers) * dim;
        rowgrad[r * width + col] = 0.f;
        rowgrad[(batch + r) * width + col] = 0.f;
        rowgrad[(2 * batch + r) * width + col] = ds;
    }
}

__global__ __launch_bounds__(kBlockThreads) void hem_score_fwd_kernel(LayerPtrs layers, int n_layers, int dim,
                                                                      const int64_t* __restrict__ rows, const int64_t* __restrict__ items,
                                                                      const float* __restrict__ bias, float lam, float* __restrict__ scores,
                                                                      int64_t batch, const int64_t* __restrict__ rows_upper) {
    const int lane = threadIdx.x & 63;
    for (int64_t r = global_wave_id(); r < batch; r += global_wave_count()) {
        float acc = 0.f;
        for (int l = 0; l < n_layers; ++l) {
            const auto [xu, xq, xi, u, q, it] = batch_row(layers, l, rows, rows_upper, batch, r);
            if (it < 0 || (u < 0 && q < 0)) continue;       // an isolated item (or both other rows zero): the layer adds nothing
            const float wu = u < 0 ? 0.f : 1.f - lam, wq = q < 0 ? 0.f : lam;
            for (int c = lane; c < dim; c += kWave) {
                const float m = wq * xq[c] + wu * xu[c];
                acc += xi[c] * m;
            }
        }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) acc += __shfl_xor(acc, o);
        if (lane == 0) scores[r] = acc + bias[items[r]];
    }
}

__global__ __launch_bounds__(kBlockThreads) void hem_score_bwd_kernel(LayerPtrs layers, int n_layers, int dim,
                                                                      const int64_t* __restrict__ rows, const float* __restrict__ dscores,
                                                                      float grad_scale, float lam, float* __restrict__ rowgrad, int64_t width,
                                                                      int64_t batch, const float* __restrict__ grad_scale_device,
                                                                      const int64_t* __restrict__ rows_upper) {
    const int lane = threadIdx.x & 63;
    if (grad_scale_device != nullptr) grad_scale *= *grad_scale_device;      // the upstream gradient of the loss, still on the device (no host read, no extra launch)
    for (int64_t r = global_wave_id(); r < batch; r += global_wave_count()) {
        const float ds = dscores[r] * grad_scale;
        bias_column(rowgrad, width, n_layers, dim, batch, r, ds);
        for (int l = 0; l < n_layers; ++l) {
            const auto [pu, pq, pi, u, q, it] = batch_row(layers, l, rows, rows_upper, batch, r);
            for (int c = lane; c < dim; c += kWave) {
                const float xu = u < 0 ? 0.f : pu[c], xq = q < 0 ? 0.f : pq[c], xi = it < 0 ? 0.f : pi[c];
                const int64_t col = static_cast<int64_t>(l) * dim + c;
                rowgrad[r * width + col] = ds * (1.f - lam) * xi;
                rowgrad[(batch + r) * width + col] = ds * lam * xi;
                rowgrad[(2 * batch + r) * width + col] = ds * (lam * xq + (1.f - lam) * xu);
            }
        }
    }
}

// ================================================================================================
// The cosine head (Gs.Prediction.use_cosine_similarity, Models/PredictionLayers.py:38-40): the same rows, the same addressing, but the score is
//   c = (a . m) / (max(||a||, eps) max(||m||, eps)) + bias[item],   a = [X_0 | .. | X_L][item],  m = lam a[query] + (1 - lam) a[user],  eps = 1e-8
// (torch.cosine_similarity).  The norms run over the WHOLE concatenated row: an isolated node's zero rows above layer 0 add nothing to the sums but the other
// rows' squares still count, so no layer is skipped.  fwd leaves the three sums of a row in stats[r] = {a.m, ||a||^2, ||m||^2, 0} (16 B per row); bwd reads them
// and every column's three outputs follow from a[c] and m[c] alone.  torch clamps the norm's VALUE and differentiates the unclamped norm (d||a||/da = a / ||a||, 0 at a = 0):
//   dc/da = m / (na nm) - c a / (na ||a||),   dc/dm = a / (na nm) - c m / (nm ||m||)      (second terms 0 for a zero row; = c a / na^2 wherever ||a|| >= eps)
//   rowgrad[0B + r] = ds (1 - lam) dc/dm,  rowgrad[1B + r] = ds lam dc/dm,  rowgrad[2B + r] = ds dc/da  - the layout of hem_score_bwd_kernel, bias column included.
// ================================================================================================
constexpr float kCosineEps = 1e-8f;

__global__ __launch_bounds__(kBlockThreads) void hem_cosine_fwd_kernel(LayerPtrs layers, int n_layers, int dim,
                                                                       const int64_t* __restrict__ rows, const int64_t* __restrict__ items,
                                                                       const float* __restrict__ bias, float lam, float* __restrict__ scores,
                                                                       float4* __restrict__ stats, int64_t batch, const int64_t* __restrict__ rows_upper) {
    const int lane = threadIdx.x & 63;
    for (int64_t r = global_wave_id(); r < batch; r += global_wave_count()) {
        float dot = 0.f, aa = 0.f, mm = 0.f;
        for (int l = 0; l < n_layers; ++l) {
            const auto [pu, pq, pi, u, q, it] = batch_row(layers, l, rows, rows_upper, batch, r);
            for (int c = lane; c < dim; c += kWave) {
                const float xu = u < 0 ? 0.f : pu[c], xq = q < 0 ? 0.f : pq[c], a = it < 0 ? 0.f : pi[c];
                const float m = lam * xq + (1.f - lam) * xu;
                dot += a * m;
                aa += a * a;
                mm += m * m;
            }
        }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) dot += __shfl_xor(dot, o);
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) aa += __shfl_xor(aa, o);
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) mm += __shfl_xor(mm, o);
        if (lane == 0) {
            const float na = fmaxf(sqrtf(aa), kCosineEps), nm = fmaxf(sqrtf(mm), kCosineEps);
            scores[r] = dot / (na * nm) + bias[items[r]];
            stats[r] = make_float4(dot, aa, mm, 0.f);
        }
    }
}

__global__ __launch_bounds__(kBlockThreads) void hem_cosine_bwd_kernel(LayerPtrs layers, int n_layers, int dim,
                                                                       const int64_t* __restrict__ rows, const float* __restrict__ dscores,
                                                                       const float4* __restrict__ stats, float grad_scale, float lam,
                                                                       float* __restrict__ rowgrad, int64_t width, int64_t batch,
                                                                       const float* __restrict__ grad_scale_device, const int64_t* __restrict__ rows_upper) {
    const int lane = threadIdx.x & 63;
    if (grad_scale_device != nullptr) grad_scale *= *grad_scale_device;
    for (int64_t r = global_wave_id(); r < batch; r += global_wave_count()) {
        const float ds = dscores[r] * grad_scale;
        bias_column(rowgrad, width, n_layers, dim, batch, r, ds);
        const float4 st = stats[r];
        const float ra = sqrtf(st.y), rm = sqrtf(st.z);
        const float na = fmaxf(ra, kCosineEps), nm = fmaxf(rm, kCosineEps);
        const float cross = 1.f / (na * nm);
        const float cosv = st.x * cross;
        const float ka = ra > 0.f ? cosv / na / ra : 0.f, km = rm > 0.f ? cosv / nm / rm : 0.f;      // (ra >= sqrt(smallest denormal) = 3.7e-23 where it is not 0: no overflow)
        for (int l = 0; l < n_layers; ++l) {
            const auto [pu, pq, pi, u, q, it] = batch_row(layers, l, rows, rows_upper, batch, r);
            for (int c = lane; c < dim; c += kWave) {
                const float xu = u < 0 ? 0.f : pu[c], xq = q < 0 ? 0.f : pq[c], a = it < 0 ? 0.f : pi[c];
                const float m = lam * xq + (1.f - lam) * xu;
                const float dm = ds * (a * cross - km * m);
                const int64_t col = static_cast<int64_t>(l) * dim + c;
                rowgrad[r * width + col] = (1.f - lam) * dm;
                rowgrad[(batch + r) * width + col] = lam * dm;
                rowgrad[(2 * batch + r) * width + col] = ds * (m * cross - ka * a);
            }
        }
    }
}

constexpr int kScatterThreads = 1024;

// Mean binary cross-entropy with logits over a batch and its gradient, one workgroup, fixed reduction tree
// (nn.BCEWithLogitsLoss(), Main.py:191): loss = mean(max(s,0) - s*y + log1p(exp(-|s|))), dscores = (sigmoid(s) - y) / n.
__global__ __launch_bounds__(kScatterThreads) void bce_with_logits_kernel(const float* __restrict__ scores, const float* __restrict__ labels, int n,
                                                                          float* __restrict__ loss, float* __restrict__ dscores) {
    __shared__ float part[kScatterThreads];
    float acc = 0.f;
    const float inv_n = 1.f / static_cast<float>(n);
    for (int k = threadIdx.x; k < n; k += kScatterThreads) {
        const float sc = scores[k], y = labels[k];
        const float e = expf(-fabsf(sc));
        acc += fmaxf(sc, 0.f) - sc * y + log1pf(e);
        const float sig = sc >= 0.f ? 1.f / (1.f + e) : e / (1.f + e);
        dscores[k] = (sig - y) * inv_n;
    }
    part[threadIdx.x] = acc;
    __syncthreads();
    for (int off = kScatterThreads / 2; off > 0; off >>= 1) {
        if (static_cast<int>(threadIdx.x) < off) part[threadIdx.x] += part[threadIdx.x + off];
        __syncthreads();
    }
    if (threadIdx.x == 0) *loss = part[0] * inv_n;
}

// Ranking losses over a batch laid out as P positives followed by P*k negatives, the negatives of positive p at P + p*k .. P + (p+1)*k - 1 (collate_fn,
// device_batches, ihg_device_batch), and d loss / d scores, one workgroup, no atomics.
//   BPR      x_pj = s_pj - s_p;  loss = (1 / (P k)) sum_p sum_j softplus(x_pj);  ds_pj = sigmoid(x_pj) / (P k);  ds_p = -sum_j ds_pj
//   SOFTMAX  m_p = max(s_p, s_pj);  e_p = exp(s_p - m_p), e_pj = exp(s_pj - m_p);  N_p = sum_j e_pj;  Z_p = e_p + N_p;
//            loss = (1 / P) sum_p ((m_p - s_p) + log Z_p);  ds_pj = (e_pj / Z_p) / P;  ds_p = -(N_p / Z_p) / P   (= (e_p / Z_p - 1) / P without its cancellation)
// A THREAD OWNS A GROUP and loops over its k negatives, j ascending; a thread takes groups threadIdx.x, threadIdx.x + 1024, ... in that order and adds their loss
// terms to its own partial sum, and the 1,024 partial sums go through bce_with_logits_kernel's tree.  Chosen over a sub-wave of lanes per group: at the working
// point (100 groups of 10) the launch is the cost either way, k is arbitrary (a lane width would have to loop as well), and sums in plain j order need no
// cross-lane step whose order depends on a lane width - so every sum's order is a function of (P, k) alone and the results are bitwise repeatable.
constexpr int kLossBpr = IHG_LOSS_BPR, kLossSoftmax = IHG_LOSS_SOFTMAX;

template <int KIND>
__global__ __launch_bounds__(kScatterThreads) void ranking_loss_kernel(const float* __restrict__ scores, int positives, int k, float* __restrict__ loss,
                                                                       float* __restrict__ dscores) {
    __shared__ float part[kScatterThreads];
    float acc = 0.f;
    const float inv_p = 1.f / static_cast<float>(positives);
    const float inv_n = 1.f / static_cast<float>(static_cast<int64_t>(positives) * k);
    for (int p = threadIdx.x; p < positives; p += kScatterThreads) {
        const float sp = scores[p];
        const int64_t first = positives + static_cast<int64_t>(p) * k;      // (< positives * (1 + k) <= INT32_MAX: checked by the entry)
        if constexpr (KIND == kLossBpr) {
            float dsum = 0.f;
            for (int j = 0; j < k; ++j) {
                const float x = scores[first + j] - sp;
                const float e = expf(-fabsf(x));
                acc += fmaxf(x, 0.f) + log1pf(e);
                const float sig = x >= 0.f ? 1.f / (1.f + e) : e / (1.f + e);
                const float d = sig * inv_n;
                dscores[first + j] = d;
                dsum += d;
            }
            dscores[p] = -dsum;
        } else {
            float m = sp;
            for (int j = 0; j < k; ++j) m = fmaxf(m, scores[first + j]);
            float negatives = 0.f;
            for (int j = 0; j < k; ++j) negatives += expf(scores[first + j] - m);
            const float z = expf(sp - m) + negatives;
            acc += (m - sp) + logf(z);
            for (int j = 0; j < k; ++j) dscores[first + j] = expf(scores[first + j] - m) / z * inv_p;      // (the same expf of the same argument as above: the same bits)
            dscores[p] = -(negatives / z) * inv_p;
        }
    }
    part[threadIdx.x] = acc;
    __syncthreads();
    for (int off = kScatterThreads / 2; off > 0; off >>= 1) {
        if (static_cast<int>(threadIdx.x) < off) part[threadIdx.x] += part[threadIdx.x + off];
        __syncthreads();
    }
    if (threadIdx.x == 0) *loss = part[0] * (KIND == kLossBpr ? inv_n : inv_p);
}

// Hard negatives (dynamic negative sampling): a batch of P positives followed by the M pool candidates of positive p at P + p*M .. P + (p+1)*M - 1; the k candidates of a
// group that come first by (score descending, pool position ascending) are its negatives, and the loss is bce_with_logits_kernel's (KIND = IHG_LOSS_BCE: labels 1 / 0, mean
// over P (1 + k)) or ranking_loss_kernel's over the positive and those k.  Score order is the order of the monotone uint32 key of the float's bits (score_key): a strict
// total order over every bit pattern, so with the position as the tie-break the M ranks of a group are a permutation of 0 .. M-1 and exactly k candidates have rank < k,
// NaNs or not.
// A WAVE OWNS A GROUP (wave w of the one workgroup takes groups w, w + 16, ...; every wave makes the same number of trips, so the barriers below are met by all):
//   1. lane l owns candidates l, l + 64, .. (at most 4): their keys go to LDS, and the lane counts over all M keys how many come before each of its own - the rank;
//   2. rank < k: selected[p][rank] = the candidate's pool position, and its score goes to LDS slot `rank`;
//   3. the group's sums run over the slots in RANK order - lane l adds slots l, l + 64, .. ascending, then the xor butterfly 32, 16, .. 1 - so their order is a function of k
//      alone, whichever lanes held the selected candidates;
//   4. every lane writes dscores of its own candidates (the same function of the same arguments as in 3: the same bits), +0.0 where the rank is >= k.
// A wave adds its groups' terms in trip order; the 16 partial sums go through a four-level tree.  No atomics; two launches on the same input agree bit for bit.
constexpr int kLossBce = IHG_LOSS_BCE;
constexpr int kPoolMax = 256;
constexpr int kLossWaves = kScatterThreads / kWave;

__device__ __forceinline__ uint32_t score_key(float s) {
    const uint32_t bits = __float_as_uint(s);
    return (bits & 0x80000000u) ? ~bits : (bits | 0x80000000u);
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// softplus(x) and sigmoid(x) as bce_with_logits_kernel / ranking_loss_kernel form them
__device__ __forceinline__ float softplus_term(float x) { return fmaxf(x, 0.f) + log1pf(expf(-fabsf(x))); }
__device__ __forceinline__ float sigmoid_of(float x) {
    const float e = expf(-fabsf(x));
    return x >= 0.f ? 1.f / (1.f + e) : e / (1.f + e);
}

// rank[t] += how many of keys[0 .. pool) come before the lane's candidate t (key own[t] at pool position lane + 64 t): a greater key, or the same key at a lower position.
// OWNED = the candidates a lane holds (1 up to a pool of 64, 2 up to 128, else 4): a pool of 50 pays for one comparison per key, not four; the key loads of four
// rounds are issued together (every lane reads the same address: a broadcast).
template <int OWNED>
__device__ __forceinline__ void count_before(const uint32_t* keys, int pool, int lane, const uint32_t (&own)[4], int (&rank)[4]) {
#pragma unroll 4
    for (int j = 0; j < pool; ++j) {
        const uint32_t other = keys[j];
#pragma unroll
        for (int t = 0; t < OWNED; ++t) rank[t] += (other > own[t] || (other == own[t] && j < lane + t * kWave)) ? 1 : 0;
    }
}

template <int KIND>
__global__ __launch_bounds__(kScatterThreads) void hard_negative_loss_kernel(const float* __restrict__ scores, int positives, int pool, int keep, float* __restrict__ loss,
                                                                             float* __restrict__ dscores, int32_t* __restrict__ selected) {
    __shared__ uint32_t keys[kLossWaves][kPoolMax];
    __shared__ float kept[kLossWaves][kPoolMax];
    __shared__ float part[kLossWaves];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int owned = (pool + kWave - 1) / kWave;                           // candidates per lane, <= 4
    const float inv_p = 1.f / static_cast<float>(positives);
    const float inv_n = 1.f / static_cast<float>(static_cast<int64_t>(positives) * (KIND == kLossBce ? keep + 1 : keep));
    float acc = 0.f;
    for (int first = 0; first < positives; first += kLossWaves) {
        const int p = first + wave;
        const bool active = p < positives;
        const int64_t base = positives + static_cast<int64_t>(active ? p : 0) * pool;      // (< positives * (1 + pool) <= INT32_MAX: checked by the entry)
        float mine[4] = {0.f, 0.f, 0.f, 0.f};
        if (active) {
            for (int t = 0; t < owned; ++t) {
                const int c = lane + t * kWave;
                if (c < pool) {
                    mine[t] = scores[base + c];
                    keys[wave][c] = score_key(mine[t]);
                }
            }
        }
        __syncthreads();
        int rank[4] = {0, 0, 0, 0};
        if (active) {
            uint32_t own[4] = {0u, 0u, 0u, 0u};
            for (int t = 0; t < owned; ++t) own[t] = (lane + t * kWave < pool) ? keys[wave][lane + t * kWave] : 0u;
            if (owned == 1) count_before<1>(keys[wave], pool, lane, own, rank);
            else if (owned == 2) count_before<2>(keys[wave], pool, lane, own, rank);
            else count_before<4>(keys[wave], pool, lane, own, rank);
            for (int t = 0; t < owned; ++t) {
                const int c = lane + t * kWave;
                if (c < pool && rank[t] < keep) {
                    selected[static_cast<int64_t>(p) * keep + rank[t]] = c;
                    kept[wave][rank[t]] = mine[t];
                }
            }
        }
        __syncthreads();
        if (active) {
            const float sp = scores[p];
            if constexpr (KIND == kLossSoftmax) {
                float m = sp;
                for (int r = lane; r < keep; r += kWave) m = fmaxf(m, kept[wave][r]);
#pragma unroll
                for (int o = 32; o >= 1; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
                float negatives = 0.f;
                for (int r = lane; r < keep; r += kWave) negatives += expf(kept[wave][r] - m);
                negatives = wave_sum(negatives);
                const float z = expf(sp - m) + negatives;
                acc += (m - sp) + logf(z);
                for (int t = 0; t < owned; ++t) {
                    const int c = lane + t * kWave;
                    if (c < pool) dscores[base + c] = rank[t] < keep ? expf(mine[t] - m) / z * inv_p : 0.f;
                }
                if (lane == 0) dscores[p] = -(negatives / z) * inv_p;
            } else if constexpr (KIND == kLossBpr) {
                float terms = 0.f, dsum = 0.f;
                for (int r = lane; r < keep; r += kWave) {
                    const float x = kept[wave][r] - sp;
                    terms += softplus_term(x);
                    dsum += sigmoid_of(x) * inv_n;
                }
                acc += wave_sum(terms);
                dsum = wave_sum(dsum);
                for (int t = 0; t < owned; ++t) {
                    const int c = lane + t * kWave;
                    if (c < pool) dscores[base + c] = rank[t] < keep ? sigmoid_of(mine[t] - sp) * inv_n : 0.f;
                }
                if (lane == 0) dscores[p] = -dsum;
            } else {
                float terms = 0.f;
                for (int r = lane; r < keep; r += kWave) terms += softplus_term(kept[wave][r]);      // label 0: max(s, 0) + log1p(exp(-|s|))
                acc += wave_sum(terms) + ((fmaxf(sp, 0.f) - sp) + log1pf(expf(-fabsf(sp))));          // label 1: max(s, 0) - s + log1p(exp(-|s|)), the positive added last
                for (int t = 0; t < owned; ++t) {
                    const int c = lane + t * kWave;
                    if (c < pool) dscores[base + c] = rank[t] < keep ? sigmoid_of(mine[t]) * inv_n : 0.f;
                }
                if (lane == 0) dscores[p] = (sigmoid_of(sp) - 1.f) * inv_n;
            }
        }
    }
    if (lane == 0) part[wave] = acc;
    __syncthreads();
    for (int off = kLossWaves / 2; off > 0; off >>= 1) {
        if (static_cast<int>(threadIdx.x) < off) part[threadIdx.x] += part[threadIdx.x + off];
        __syncthreads();
    }
    if (threadIdx.x == 0) *loss = part[0] * (KIND == kLossSoftmax ? inv_p : inv_n);
}

// Deterministic scatter-add of a small batch of rows into a large dense matrix: dense[rows[k], :] += rowgrad[k, :], duplicates
// summed in batch order, no atomics, no sort.  One wave per batch position k: it scans rows[0..k) for an earlier occurrence of
// its destination (ballot over 64 ids at a time; the id array is a few KB and cache-resident) and retires if there is one;
// otherwise it is the leader of that destination, walks rows[k..n) in order and adds every matching batch row, then writes the
// destination row once.  O(n^2 / 64) wave-steps in total - microseconds for the few thousand rows of a training batch; replaces
// index_put_(accumulate=True) (bounds checks, device radix sort, scatter kernel).
constexpr int kScatterMax = 16384;                      // ids of one launch in 64 KiB of LDS: any single-GPU batch (3 x 1,100 rows) ...
constexpr int kScatterMaxWide = 32768;                  // ... and the wide instance (128 of gfx950's 160 KiB, one workgroup per CU) for the UNION of the ranks' batches in the
                                                        // data-parallel cotangent exchange (8 ranks x 3,300 rows = 26,400; ihgnn_amd/distributed.py: CotangentSync)

// Destination addressing: column c of batch row k goes to dense[(c / block_width) * block_stride + row * ld_dense + c % block_width]
// (block_width = width, block_stride = 0 is a plain matrix; block_width = d, block_stride = N*d lands layer l's columns in its own
// contiguous [N, d] matrix); an optional last column goes to tail[row - tail_row_offset] (the bias gradient).
// COMBINE: nothing is scattered; the sum over a destination's batch rows replaces the FIRST of them in rowgrad itself (a row
// is read by the wave of its destination's first occurrence only, which is also its only writer) and leader[k] says whether
// batch row k is such a first occurrence.  batch_rows_add_kernel then adds leader rows wherever they are needed.
template <bool COMBINE, int CAP = kScatterMax>
__global__ __launch_bounds__(kBlockThreads) void batch_scatter_kernel(float* __restrict__ rowgrad, int64_t ld_rowgrad, int width,
                                                                      const int64_t* __restrict__ rows, int n, float* __restrict__ dense,
                                                                      int64_t ld_dense, int block_width, int64_t block_stride,
                                                                      float* __restrict__ tail, int64_t tail_row_offset, int64_t tail_rows,
                                                                      int32_t* __restrict__ leader, int block_rows) {
    // block_rows: rows of different consecutive blocks of this many batch rows never share a destination (the user / query / item
    // thirds of a batch address disjoint node ranges), so a wave only scans its own block; n = one block is the general case.
    // A WORKGROUP belongs to one block (blockIdx.y) and keeps only that block's ids in LDS (CAP >= block_rows): a third of the fill and of the LDS of the whole list - the
    // union of eight ranks' batches (3 x 8,800 rows) runs on the 64 KiB instance, two workgroups per CU.  A NEGATIVE id is a row that takes no part (its gradient was
    // already summed into another row - a rank's own duplicates, combined before the exchange): never a leader, never matched.
    __shared__ int32_t key[CAP];
    const int lo = static_cast<int>(blockIdx.y) * block_rows;
    const int hi = lo + block_rows < n ? lo + block_rows : n;
    for (int k = lo + threadIdx.x; k < hi; k += kBlockThreads) key[k - lo] = static_cast<int32_t>(rows[k]);
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int wave = static_cast<int>(blockIdx.x) * kWavesPerBlock + (threadIdx.x >> 6);
    for (int64_t k = lo + wave; k < hi; k += static_cast<int64_t>(gridDim.x) * kWavesPerBlock) {
        const int32_t mine = key[k - lo];
        if (mine < 0) {
            if (COMBINE && lane == 0) leader[k] = 0;
            continue;
        }
        bool follower = false;
        for (int base = lo; base < k; base += kWave) {
            const int j = base + lane;
            if (__ballot(j < k && key[j - lo] == mine) != 0ull) { follower = true; break; }
        }
        if (COMBINE && lane == 0) leader[k] = follower ? 0 : 1;
        if (follower) continue;
        for (int c0 = 0; c0 < width; c0 += 4 * kWave) {
            float acc[4] = {0.f, 0.f, 0.f, 0.f};
            for (int base = static_cast<int>(k) & ~(kWave - 1); base < hi; base += kWave) {
                const int j = base + lane;
                unsigned long long mask = __ballot(j >= k && j < hi && key[j - lo] == mine);
                while (mask != 0ull) {
                    // up to 16 members per trip: all their loads are issued before the first add (a hot destination - a
                    // popular query - can own hundreds of batch rows); absent slots add an exact 0
                    constexpr int MEMBERS = 16;
                    float v[MEMBERS][4];
#pragma unroll
                    for (int u = 0; u < MEMBERS; ++u) {
                        const bool have = mask != 0ull;
                        const int bit = have ? __ffsll(static_cast<long long>(mask)) - 1 : 0;
                        if (have) mask &= mask - 1;
                        const float* src = rowgrad + static_cast<int64_t>(base + bit) * ld_rowgrad;
#pragma unroll
                        for (int q = 0; q < 4; ++q) {
                            const int c = c0 + q * kWave + lane;
                            v[u][q] = (have && c < width) ? src[c] : 0.f;
                        }
                    }
#pragma unroll
                    for (int u = 0; u < MEMBERS; ++u)
#pragma unroll
                        for (int q = 0; q < 4; ++q) acc[q] += v[u][q];
                }
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int c = c0 + q * kWave + lane;
                if (c >= width) continue;
                if (COMBINE) {
                    rowgrad[k * ld_rowgrad + c] = acc[q];
                } else if (tail != nullptr && c == width - 1) {
                    const int64_t tr = static_cast<int64_t>(mine) - tail_row_offset;
                    if (tr >= 0 && tr < tail_rows) tail[tr] += acc[q];
                } else {
                    dense[(c / block_width) * block_stride + static_cast<int64_t>(mine) * ld_dense + c % block_width] += acc[q];
                }
            }
        }
    }
}

// dense[rows[k], 0:width] += src[k, 0:width] for the leader rows of a combined batch (no two leaders share a destination);
// with `tail`, the single column src[k, 0] goes to tail[rows[k] - tail_row_offset] instead.
// dense: virtual bases per node type (TypedRowsOut; a plain matrix: three equal pointers), begin1 / begin2 = first query / item row; ASSIGN: = instead of +=
template <bool ASSIGN>
__global__ __launch_bounds__(kBlockThreads) void batch_rows_add_kernel(const float* __restrict__ src, int64_t ld_src, int width,
                                                                       const int64_t* __restrict__ rows, const int32_t* __restrict__ leader, int n,
                                                                       TypedRowsOut dense, int64_t begin1, int64_t begin2, int64_t ld_dense, float* __restrict__ tail,
                                                                       int64_t tail_row_offset, int64_t tail_rows) {
    const int lane = threadIdx.x & 63;
    for (int64_t k = global_wave_id(); k < n; k += global_wave_count()) {
        if (leader[k] == 0) continue;
        const int64_t row = rows[k];
        if (row < 0) continue;                               // (an isolated node under a compact layout: its rows above layer 0 are constants)
        if (tail != nullptr) {
            const int64_t tr = row - tail_row_offset;
            if (lane == 0 && tr >= 0 && tr < tail_rows) tail[tr] += src[k * ld_src];
            continue;
        }
        float* dst = typed_base(dense, row >= begin2 ? 2 : (row >= begin1 ? 1 : 0)) + row * ld_dense;
        for (int c = lane; c < width; c += kWave) dst[c] = ASSIGN ? src[k * ld_src + c] : dst[c] + src[k * ld_src + c];
    }
}

// mask[rows[k]] = value for the k < n listed rows (the row mask of the last layer's sparse cotangent: set before its pull, cleared after)
__global__ __launch_bounds__(kBlockThreads) void mark_rows_kernel(const int64_t* __restrict__ rows64, const int32_t* __restrict__ rows32, int64_t n, uint8_t* __restrict__ mask,
                                                                  uint8_t value) {
    for (int64_t k = static_cast<int64_t>(blockIdx.x) * kBlockThreads + threadIdx.x; k < n; k += static_cast<int64_t>(gridDim.x) * kBlockThreads)
        mask[rows64 != nullptr ? rows64[k] : static_cast<int64_t>(rows32[k])] = value;
}

// rows[0 .. 3 b) = users | queries + query_row0 | items + item_row0 (the global node rows of a batch, Models/RawGnn.py:128-131: torch.cat of three index vectors + two adds)
__global__ __launch_bounds__(kBlockThreads) void batch_node_rows_kernel(const int64_t* __restrict__ users, const int64_t* __restrict__ queries, const int64_t* __restrict__ items,
                                                                        int64_t b, int64_t query_row0, int64_t item_row0, int64_t* __restrict__ rows, int32_t* __restrict__ rows32) {
    for (int64_t k = static_cast<int64_t>(blockIdx.x) * kBlockThreads + threadIdx.x; k < 3 * b; k += static_cast<int64_t>(gridDim.x) * kBlockThreads) {
        const int64_t r = k < b ? users[k] : (k < 2 * b ? queries[k - b] + query_row0 : items[k - 2 * b] + item_row0);
        rows[k] = r;
        if (rows32 != nullptr) rows32[k] = static_cast<int32_t>(r);
    }
}

// base[rows[k], 0 .. dim) = 0 for the k < n listed rows (one wave per row)
__global__ __launch_bounds__(kBlockThreads) void zero_rows_kernel(float* __restrict__ base, int64_t ld, int dim, const int64_t* __restrict__ rows, int64_t n) {
    const int lane = threadIdx.x & 63;
    for (int64_t k = global_wave_id(); k < n; k += global_wave_count())
        for (int c = lane; c < dim; c += kWave) base[rows[k] * ld + c] = 0.f;
}

// ------------------------------------------------------------------------------------------------
// Adam over a list of tensors in one launch (pointer table passed by value): a pure stream, 7 passes of 4 bytes per parameter.
// ------------------------------------------------------------------------------------------------
constexpr int kAdamMaxTensors = 24;
constexpr int kAdamChunk = 4096;                            // elements per workgroup trip

struct AdamTable {
    float* param[kAdamMaxTensors];
    const float* grad[kAdamMaxTensors];
    float* exp_avg[kAdamMaxTensors];
    float* exp_avg_sq[kAdamMaxTensors];
    int64_t chunk_begin[kAdamMaxTensors + 1];               // prefix of ceil(n / kAdamChunk)
    int64_t count[kAdamMaxTensors];
    int n_tensors;
};

// kClip: g <- g * coef first (torch.nn.utils.clip_grad_norm_ scales the gradient before Adam adds the weight-decay term); the gradient in memory is not rewritten
template <bool kClip>
__device__ __forceinline__ void adam_update(float& p, float g, float& m, float& v, float beta1, float beta2, float eps, float weight_decay,
                                            float step_size, float bias2_sqrt, float coef) {
    if (kClip) {
#pragma clang fp contract(off)                               // a product of its own: fused into the decay term's sum, coef = 1 would not give the unclipped instance's bits
        g = g * coef;
    }
    // (the decay term as the one fma the unclipped instance has always been contracted to - written out, so that the clipped instance cannot pair its product
    // with g * coef in a packed multiply and round it).  That the unclipped instance is bit for bit what `g + weight_decay * p` compiled to rests on the build
    // keeping hipcc's default -ffp-contract (fast-honor-pragmas): under -ffp-contract=off the old form rounded the product and this one does not.
    g = weight_decay != 0.f ? fmaf(weight_decay, p, g) : g;
    m = m + (g - m) * (1.f - beta1);                        // torch's lerp form
    v = beta2 * v + (1.f - beta2) * g * g;
    const float denom = sqrtf(v) / bias2_sqrt + eps;
    p = p - step_size * (m / denom);
}

// `scalars` != nullptr: {step_size, bias2_sqrt} are read from device memory at launch time (a captured launch replays with the step's own values).
// kClip: `clip` = {norm, coef} on the device (clip_record_kernel), every gradient is multiplied by coef as it is read.
template <bool kClip>
__global__ __launch_bounds__(kBlockThreads) void adam_kernel(AdamTable tab, float beta1, float beta2, float eps, float weight_decay, float step_size,
                                                             float bias2_sqrt, const float* __restrict__ scalars, const float* __restrict__ clip) {
    if (scalars != nullptr) {
        step_size = scalars[0];
        bias2_sqrt = scalars[1];
    }
    const float coef = kClip ? clip[1] : 1.f;
    const int64_t total_chunks = tab.chunk_begin[tab.n_tensors];
    for (int64_t chunk = blockIdx.x; chunk < total_chunks; chunk += gridDim.x) {
        int t = 0;
        while (chunk >= tab.chunk_begin[t + 1]) ++t;
        const int64_t base = (chunk - tab.chunk_begin[t]) * kAdamChunk;
        const int64_t n = tab.count[t];
        float* __restrict__ p = tab.param[t];
        const float* __restrict__ g = tab.grad[t];
        float* __restrict__ m = tab.exp_avg[t];
        float* __restrict__ v = tab.exp_avg_sq[t];
        const bool vec = ((reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(m) | reinterpret_cast<uintptr_t>(v)) & 15) == 0;
        if (vec && base + kAdamChunk <= n) {
#pragma unroll
            for (int k = 0; k < kAdamChunk / (4 * kBlockThreads); ++k) {
                const int64_t i = base + (threadIdx.x + k * kBlockThreads) * 4;
                v4f pv = *reinterpret_cast<const v4f*>(p + i), mv = *reinterpret_cast<const v4f*>(m + i), vv = *reinterpret_cast<const v4f*>(v + i);
                const v4f gv = *reinterpret_cast<const v4f*>(g + i);
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    float pc = pv[c], mc = mv[c], vc = vv[c];
                    adam_update<kClip>(pc, gv[c], mc, vc, beta1, beta2, eps, weight_decay, step_size, bias2_sqrt, coef);
                    pv[c] = pc; mv[c] = mc; vv[c] = vc;
                }
                *reinterpret_cast<v4f*>(p + i) = pv;
                *reinterpret_cast<v4f*>(m + i) = mv;
                *reinterpret_cast<v4f*>(v + i) = vv;
            }
        } else {
            for (int64_t i = base + threadIdx.x; i < base + kAdamChunk && i < n; i += kBlockThreads)
                adam_update<kClip>(p[i], g[i], m[i], v[i], beta1, beta2, eps, weight_decay, step_size, bias2_sqrt, coef);
        }
    }
}

// ------------------------------------------------------------------------------------------------
// Global gradient norm for clipping (torch.nn.utils.clip_grad_norm_, norm_type 2), over the table Adam takes.  One double per kAdamChunk elements: thread t adds the
// squares of elements (t + 256 k) 4 + c, k = 0 .. 3, c = 0 .. 3 of its chunk in that order (a float's square is exact in double), six xor-shuffle steps add the lanes,
// thread 0 adds the four waves in order.  A chunk's partial depends on the chunk alone - not on the grid, not on the pointer's alignment (the scalar path walks the same
// elements in the same order) - so the sum is bitwise repeatable; no atomics.
// ------------------------------------------------------------------------------------------------
struct GradNormTable {
    const float* grad[kAdamMaxTensors];
    int64_t chunk_begin[kAdamMaxTensors + 1];
    int64_t count[kAdamMaxTensors];
    int n_tensors;
};

__device__ __forceinline__ double block_sum_fixed_order(double acc) {        // every thread of the workgroup calls; the result is valid in thread 0
    __shared__ double waves[kWavesPerBlock];
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) acc += __shfl_xor(acc, o);
    if ((threadIdx.x & 63) == 0) waves[threadIdx.x >> 6] = acc;
    __syncthreads();
    double total = 0.0;
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 0; w < kWavesPerBlock; ++w) total += waves[w];
    }
    __syncthreads();                                         // (the next trip writes `waves` again)
    return total;
}

__global__ __launch_bounds__(kBlockThreads) void grad_sqnorm_partial_kernel(GradNormTable tab, double* __restrict__ partials) {
    const int64_t total_chunks = tab.chunk_begin[tab.n_tensors];
    for (int64_t chunk = blockIdx.x; chunk < total_chunks; chunk += gridDim.x) {
        int t = 0;
        while (chunk >= tab.chunk_begin[t + 1]) ++t;
        const int64_t base = (chunk - tab.chunk_begin[t]) * kAdamChunk;
        const int64_t n = tab.count[t];
        const float* __restrict__ g = tab.grad[t];
        double acc = 0.0;
        if ((reinterpret_cast<uintptr_t>(g) & 15) == 0 && base + kAdamChunk <= n) {
#pragma unroll
            for (int k = 0; k < kAdamChunk / (4 * kBlockThreads); ++k) {
                const v4f gv = *reinterpret_cast<const v4f*>(g + base + (threadIdx.x + k * kBlockThreads) * 4);
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const double x = static_cast<double>(gv[c]);
                    acc += x * x;
                }
            }
        } else {
            for (int k = 0; k < kAdamChunk / (4 * kBlockThreads); ++k) {
                const int64_t i = base + (threadIdx.x + k * kBlockThreads) * 4;
                for (int c = 0; c < 4 && i + c < n; ++c) {
                    const double x = static_cast<double>(g[i + c]);
                    acc += x * x;
                }
            }
        }
        const double total = block_sum_fixed_order(acc);
        if (threadIdx.x == 0) partials[chunk] = total;
    }
}

// one workgroup: thread t adds partials t, t + 256, ... in order, then the same wave and LDS tree
__global__ __launch_bounds__(kBlockThreads) void grad_sqnorm_finish_kernel(const double* __restrict__ partials, int64_t n_partials, double* __restrict__ sum) {
    double acc = 0.0;
    for (int64_t i = threadIdx.x; i < n_partials; i += kBlockThreads) acc += partials[i];
    const double total = block_sum_fixed_order(acc);
    if (threadIdx.x == 0) *sum = total;
}

// clip = {norm, coef}: norm = (float) sqrt(sum), coef = min(max_norm / (norm + 1e-6), 1) as torch.clamp(max=1) takes it - a NaN stays a NaN (fminf would return 1).
// stats (optional) = {largest norm so far, steps with coef < 1, steps}.  One thread, plain stores.
__global__ void clip_record_kernel(const double* __restrict__ sum, float max_norm, float* __restrict__ clip, float* __restrict__ stats) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const float norm = static_cast<float>(sqrt(*sum));
    float coef = max_norm / (norm + 1e-6f);
    coef = coef > 1.f ? 1.f : coef;
    clip[0] = norm;
    clip[1] = coef;
    if (stats != nullptr) {
        const float seen = stats[0];
        stats[0] = norm > seen ? norm : seen;
        stats[1] = stats[1] + (coef < 1.f ? 1.f : 0.f);
        stats[2] = stats[2] + 1.f;
    }
}

}  // namespace

// ------------------------------------------------------------------------------------------------
// Negative sampling on the device: `random.sample(range(n_items), k)` per positive (Dataset.py:107-109) - k DISTINCT
// items, uniform over the catalogue, the positive itself not excluded.  Counter-based generator: draw (row, slot, attempt) is a
// pure function of (seed, batch counter), so a run is reproducible whatever the launch geometry; a repeated item inside a
// sample is rejected and redrawn (k <= 16, so the check is a register scan).
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint64_t mix64(uint64_t x) {                  // splitmix64 finaliser
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

constexpr int kSampleMax = 16;
constexpr uint64_t kPositionStream = 0xA0761D6478BD642Full;             // the stream of list positions: a row's key xor this (ihg_device_batch)

__device__ __forceinline__ uint64_t sample_row_key(uint64_t seed, uint64_t counter, int64_t row) {
    return mix64(seed ^ mix64(counter)) ^ mix64(static_cast<uint64_t>(row) * 0xD1B54A32D192ED03ull);
}

// picked[0..c) = c DISTINCT values below m (c <= min(kSampleMax, m)), the draws of the stream `key` with its attempts counted from 0: the first c' <= c of
// them are what a call with c' gives.  Both streams of both kernels below come from here.
__device__ __forceinline__ void draw_distinct(uint64_t key, uint64_t m, int c, int64_t (&picked)[kSampleMax]) {
    uint64_t attempt = 0;
#pragma unroll 1
    for (int slot = 0; slot < c; ++slot) {
        int64_t value;
        bool fresh;
        do {
            const uint64_t r = mix64(key + (attempt++) * 0x2545F4914F6CDD1Dull);
            value = static_cast<int64_t>(__umul64hi(r, m));                                      // uniform on [0, m) up to 2^-64 m
            fresh = true;
            for (int j = 0; j < slot; ++j) fresh = fresh && picked[j] != value;
        } while (!fresh);
        picked[slot] = value;
    }
}

__global__ __launch_bounds__(kBlockThreads) void sample_negatives_kernel(uint64_t seed, uint64_t counter, int64_t n_rows, int64_t n_items, int k,
                                                                         int64_t* __restrict__ out) {
    for (int64_t row = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; row < n_rows; row += static_cast<int64_t>(gridDim.x) * blockDim.x) {
        int64_t picked[kSampleMax];
        draw_distinct(sample_row_key(seed, counter, row), static_cast<uint64_t>(n_items), k, picked);
        for (int slot = 0; slot < k; ++slot) out[row * k + slot] = picked[slot];
    }
}

// draw_distinct continued past kSampleMax (ihg_sample_pool): a WORKGROUP OF ONE WAVE per row.  Attempts are taken 64 at a time, lane j taking attempt base + j; a lane's
// value is fresh iff it is not in the accepted list (LDS) and no EARLIER lane of the chunk holds it - an earlier lane with the same value is either accepted or itself a
// repeat of an accepted value, so this is the sequential rule.  Slots come from the ballot's prefix count, cut at m: the first m accepted values in attempt order.
// The loop ends like draw_distinct's: m <= n_items values are there to be found (m = n_items = 256 takes about thirty chunks).
constexpr int kPoolDraws = 256;

__global__ __launch_bounds__(kWave) void sample_pool_kernel(uint64_t seed, uint64_t counter, int64_t n_rows, int64_t n_items, int m, int64_t* __restrict__ out) {
    __shared__ int64_t accepted[kPoolDraws];
    __shared__ int64_t chunk[kWave];
    const int lane = threadIdx.x;
    for (int64_t row = blockIdx.x; row < n_rows; row += gridDim.x) {
        const uint64_t key = sample_row_key(seed, counter, row);
        int count = 0;                                                   // accepted so far: the same in every lane (it follows from ballots)
        for (uint64_t base = 0; count < m; base += kWave) {
            const uint64_t r = mix64(key + (base + lane) * 0x2545F4914F6CDD1Dull);
            const int64_t value = static_cast<int64_t>(__umul64hi(r, static_cast<uint64_t>(n_items)));
            chunk[lane] = value;
            __syncthreads();                                             // (one wave: the chunk, and the list as the last round left it, are visible)
            bool fresh = true;
            for (int j = 0; j < count; ++j) fresh = fresh && accepted[j] != value;
            for (int j = 0; j < kWave; ++j) fresh = fresh && (j >= lane || chunk[j] != value);
            const unsigned long long mask = __ballot(fresh);
            const int slot = count + __popcll(mask & ((1ull << lane) - 1ull));
            if (fresh && slot < m) {
                accepted[slot] = value;
                out[row * m + slot] = value;
            }
            count += __popcll(mask);
            __syncthreads();
        }
    }
}

// sample_pool_kernel with a per-row list of values that are never accepted (ihg_sample_pool_excluding): the same wave per row, the same chunks of 64 attempts.  A lane's
// value is fresh iff it is not on the row's list (a binary search over the sorted int32 run, every lane for its own value), not in the accepted list and not held by an
// EARLIER lane of the chunk.  An earlier lane with the same value is accepted, a repeat of an accepted value, or itself on the list - and then so is this lane's value,
// which its own search has found: the sequential rule again.  With an empty list the search finds nothing and this is sample_pool_kernel to the bit.  A row whose list id
// lies outside [0, n_lists) has an empty list, and list_ptr is not read for it.  The loop ends because the entry point has been promised m + (longest list) <= n_items.
__global__ __launch_bounds__(kWave) void sample_pool_excluding_kernel(uint64_t seed, uint64_t counter, int64_t n_rows, int64_t n_items, int m,
                                                                      const int64_t* __restrict__ list_of_row, int64_t n_lists, const int64_t* __restrict__ list_ptr,
                                                                      const int32_t* __restrict__ list_items, int64_t* __restrict__ out) {
    __shared__ int64_t accepted[kPoolDraws];
    __shared__ int64_t chunk[kWave];
    const int lane = threadIdx.x;
    for (int64_t row = blockIdx.x; row < n_rows; row += gridDim.x) {
        const uint64_t key = sample_row_key(seed, counter, row);
        const int64_t which = list_of_row[row];
        const bool listed_row = which >= 0 && which < n_lists;
        const int64_t first = listed_row ? list_ptr[which] : 0;
        const int64_t len = listed_row ? list_ptr[which + 1] - first : 0;
        const int32_t* const list = list_items + first;                  // list[0 .. len): ascending, distinct
        int count = 0;                                                   // accepted so far: the same in every lane (it follows from ballots)
        for (uint64_t base = 0; count < m; base += kWave) {
            const uint64_t r = mix64(key + (base + lane) * 0x2545F4914F6CDD1Dull);
            const int64_t value = static_cast<int64_t>(__umul64hi(r, static_cast<uint64_t>(n_items)));
            chunk[lane] = value;
            __syncthreads();                                             // (one wave: the chunk, and the list as the last round left it, are visible)
            int64_t lo = 0, hi = len;                                    // the first entry >= value
            while (lo < hi) {
                const int64_t mid = (lo + hi) >> 1;
                if (static_cast<int64_t>(list[mid]) < value) lo = mid + 1; else hi = mid;
            }
            bool fresh = !(lo < len && static_cast<int64_t>(list[lo]) == value);
            for (int j = 0; j < count; ++j) fresh = fresh && accepted[j] != value;
            for (int j = 0; j < kWave; ++j) fresh = fresh && (j >= lane || chunk[j] != value);
            const unsigned long long mask = __ballot(fresh);
            const int slot = count + __popcll(mask & ((1ull << lane) - 1ull));
            if (fresh && slot < m) {
                accepted[slot] = value;
                out[row * m + slot] = value;
            }
            count += __popcll(mask);
            __syncthreads();
        }
    }
}

// sample_pool_excluding_kernel with a weighted value (ihg_sample_pool_weighted): the same wave per row, the same chunks of 64 attempts, the same freshness rule.  The one
// new step: a lane's 64 random bits become a threshold t = umulhi(r, total) in [0, total), and its value is the one i with cum[i] <= t < cum[i + 1] - a binary search over
// cum [n_items + 1] that keeps cum[lo] <= t < cum[hi] from (0, n_items) on, so that every index it reads lies in [0, n_items] whatever the table holds.  With cum[i] = i
// the search returns t itself and this is sample_pool_excluding_kernel to the bit.  list_of_row == nullptr (n_lists == 0): no row has a list and no list pointer is read.
// The loop ends because cum is strictly ascending (every item can be drawn) and the entry point has been promised m + (longest list) <= n_items.
__global__ __launch_bounds__(kWave) void sample_pool_weighted_kernel(uint64_t seed, uint64_t counter, int64_t n_rows, int64_t n_items, int m,
                                                                     const int64_t* __restrict__ cum, uint64_t total, const int64_t* __restrict__ list_of_row,
                                                                     int64_t n_lists, const int64_t* __restrict__ list_ptr, const int32_t* __restrict__ list_items,
                                                                     int64_t* __restrict__ out) {
    __shared__ int64_t accepted[kPoolDraws];
    __shared__ int64_t chunk[kWave];
    const int lane = threadIdx.x;
    for (int64_t row = blockIdx.x; row < n_rows; row += gridDim.x) {
        const uint64_t key = sample_row_key(seed, counter, row);
        const int64_t which = list_of_row != nullptr ? list_of_row[row] : -1;
        const bool listed_row = which >= 0 && which < n_lists;
        const int64_t first = listed_row ? list_ptr[which] : 0;
        const int64_t len = listed_row ? list_ptr[which + 1] - first : 0;
        const int32_t* const list = list_items + first;                  // list[0 .. len): ascending, distinct (never read when len == 0)
        int count = 0;                                                   // accepted so far: the same in every lane (it follows from ballots)
        for (uint64_t base = 0; count < m; base += kWave) {
            const uint64_t r = mix64(key + (base + lane) * 0x2545F4914F6CDD1Dull);
            const int64_t t = static_cast<int64_t>(__umul64hi(r, total));                        // < total < 2^63
            int64_t below = 0, above = n_items;                          // cum[below] <= t < cum[above]
            while (above - below > 1) {
                const int64_t mid = (below + above) >> 1;
                if (cum[mid] <= t) below = mid; else above = mid;
            }
            const int64_t value = below;
            chunk[lane] = value;
            __syncthreads();                                             // (one wave: the chunk, and the list as the last round left it, are visible)
            int64_t lo = 0, hi = len;                                    // the first entry >= value
            while (lo < hi) {
                const int64_t mid = (lo + hi) >> 1;
                if (static_cast<int64_t>(list[mid]) < value) lo = mid + 1; else hi = mid;
            }
            bool fresh = !(lo < len && static_cast<int64_t>(list[lo]) == value);
            for (int j = 0; j < count; ++j) fresh = fresh && accepted[j] != value;
            for (int j = 0; j < kWave; ++j) fresh = fresh && (j >= lane || chunk[j] != value);
            const unsigned long long mask = __ballot(fresh);
            const int slot = count + __popcll(mask & ((1ull << lane) - 1ull));
            if (fresh && slot < m) {
                accepted[slot] = value;
                out[row * m + slot] = value;
            }
            count += __popcll(mask);
            __syncthreads();
        }
    }
}

// One thread per positive writes its column of the pack and the k = k_rand + k_logged columns of its negatives (header: ihg_device_batch).
__global__ __launch_bounds__(kBlockThreads) void device_batch_kernel(uint64_t seed, uint64_t counter, const int64_t* __restrict__ pos_triples,
                                                                     const int64_t* __restrict__ edge_ids, int64_t n, const int32_t* __restrict__ pair_of_edge,
                                                                     const int64_t* __restrict__ neg_ptr, const int32_t* __restrict__ neg_items, int64_t n_items,
                                                                     int k_rand, int k_logged, int64_t* __restrict__ pack) {
    const int k = k_rand + k_logged;
    const int64_t width = n * (1 + k);
    int64_t* const users = pack;
    int64_t* const queries = pack + width;
    int64_t* const items = pack + 2 * width;
    int64_t* const flags = pack + 3 * width;
    for (int64_t row = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; row < n; row += static_cast<int64_t>(gridDim.x) * blockDim.x) {
        const int64_t edge = edge_ids[row];
        const int64_t user = pos_triples[3 * edge], query = pos_triples[3 * edge + 1];
        users[row] = user;
        queries[row] = query;
        items[row] = pos_triples[3 * edge + 2];
        flags[row] = 1;

        int64_t list = 0, len = 0;                                       // the pair's logged negatives: neg_items[list .. list + len)
        if (k_logged > 0) {
            const int32_t pair = pair_of_edge[edge];
            list = neg_ptr[pair];
            len = neg_ptr[pair + 1] - list;
        }
        const bool enough = len >= k_logged;
        const int n_random = enough ? k_rand : k - static_cast<int>(len);
        const int n_listed = k - n_random;                               // k_logged drawn positions, or the whole (shorter) list
        const int first_random = enough ? n_listed : 0;                  // drawn logged items come first; a short list comes last, in file order
        const int first_listed = enough ? 0 : n_random;
        const int64_t col0 = n + row * k;
        const uint64_t key = sample_row_key(seed, counter, row);
        int64_t picked[kSampleMax];
        if (enough && n_listed > 0) draw_distinct(key ^ kPositionStream, static_cast<uint64_t>(len), n_listed, picked);
        for (int j = 0; j < n_listed; ++j) items[col0 + first_listed + j] = neg_items[list + (enough ? picked[j] : j)];
        draw_distinct(key, static_cast<uint64_t>(n_items), n_random, picked);
        for (int j = 0; j < n_random; ++j) items[col0 + first_random + j] = picked[j];
        for (int j = 0; j < k; ++j) {
            users[col0 + j] = user;
            queries[col0 + j] = query;
            flags[col0 + j] = 0;
        }
    }
}

extern "C" {

int ihg_sample_negatives(uint64_t seed, uint64_t counter, int64_t n_rows, int64_t n_items, int32_t k, int64_t* out, ihg_stream_t stream) {
    if (n_rows < 0 || n_items <= 0 || k <= 0 || k > kSampleMax || k > n_items)
        return fail(IHG_ERR_INVALID, "ihg_sample_negatives: need 1 <= k <= min(%d, n_items)", kSampleMax);
    if (n_rows == 0) return IHG_OK;
    if (out == nullptr) return fail(IHG_ERR_INVALID, "ihg_sample_negatives: null pointer");
    const int grid = static_cast<int>(std::min<int64_t>((n_rows + kBlockThreads - 1) / kBlockThreads, kMaxBlocks));
    hipLaunchKernelGGL(sample_negatives_kernel, dim3(grid), dim3(kBlockThreads), 0, static_cast<hipStream_t>(stream), seed, counter, n_rows, n_items, k, out);
    return check_launch("ihg_sample_negatives");
}

int ihg_sample_pool(uint64_t seed, uint64_t counter, int64_t n_rows, int64_t n_items, int32_t m, int64_t* out, ihg_stream_t stream) {
    if (n_rows < 0 || n_items <= 0 || m < 1 || m > kPoolDraws || m > n_items)
        return fail(IHG_ERR_INVALID, "ihg_sample_pool: need 1 <= m <= min(%d, n_items), got m = %d and n_items = %lld", kPoolDraws, m, (long long)n_items);
    if (n_rows == 0) return IHG_OK;
    if (out == nullptr) return fail(IHG_ERR_INVALID, "ihg_sample_pool: null pointer");
    const int grid = static_cast<int>(std::min<int64_t>(n_rows, static_cast<int64_t>(kMaxBlocks) * kWavesPerBlock));
    hipLaunchKernelGGL(sample_pool_kernel, dim3(grid), dim3(kWave), 0, static_cast<hipStream_t>(stream), seed, counter, n_rows, n_items, static_cast<int>(m), out);
    return check_launch("ihg_sample_pool");
}

int ihg_sample_pool_excluding(uint64_t seed, uint64_t counter, int64_t n_rows, int64_t n_items, int32_t m, const int64_t* list_of_row, int64_t n_lists,
                              const int64_t* list_ptr, const int32_t* list_items, int64_t max_list_len, int64_t* out, ihg_stream_t stream) {
    if (n_rows < 0 || n_items <= 0 || m < 1 || m > kPoolDraws || m > n_items)
        return fail(IHG_ERR_INVALID, "ihg_sample_pool_excluding: need 1 <= m <= min(%d, n_items), got m = %d and n_items = %lld", kPoolDraws, m, (long long)n_items);
    if (n_lists < 1 || max_list_len < 0)
        return fail(IHG_ERR_INVALID, "ihg_sample_pool_excluding: need n_lists >= 1 and max_list_len >= 0, got n_lists = %lld and max_list_len = %lld", (long long)n_lists,
                    (long long)max_list_len);
    if (max_list_len > n_items - m)                                      // (the row with the longest list would have fewer than m values to find: its loop would not end)
        return fail(IHG_ERR_INVALID, "ihg_sample_pool_excluding: need m + max_list_len <= n_items, got m = %d, max_list_len = %lld and n_items = %lld", m,
                    (long long)max_list_len, (long long)n_items);
    if (n_rows == 0) return IHG_OK;
    if (list_of_row == nullptr || list_ptr == nullptr || list_items == nullptr || out == nullptr) return fail(IHG_ERR_INVALID, "ihg_sample_pool_excluding: null pointer");
    const int grid = static_cast<int>(std::min<int64_t>(n_rows, static_cast<int64_t>(kMaxBlocks) * kWavesPerBlock));
    hipLaunchKernelGGL(sample_pool_excluding_kernel, dim3(grid), dim3(kWave), 0, static_cast<hipStream_t>(stream), seed, counter, n_rows, n_items, static_cast<int>(m),
                       list_of_row, n_lists, list_ptr, list_items, out);
    return check_launch("ihg_sample_pool_excluding");
}

int ihg_sample_pool_weighted(uint64_t seed, uint64_t counter, int64_t n_rows, int64_t n_items, int32_t m, const int64_t* cum, int64_t total, const int64_t* list_of_row,
                             int64_t n_lists, const int64_t* list_ptr, const int32_t* list_items, int64_t max_list_len, int64_t* out, ihg_stream_t stream) {
    if (n_rows < 0 || n_items <= 0 || m < 1 || m > kPoolDraws || m > n_items)
        return fail(IHG_ERR_INVALID, "ihg_sample_pool_weighted: need 1 <= m <= min(%d, n_items), got m = %d and n_items = %lld", kPoolDraws, m, (long long)n_items);
    if (total < n_items)                                                 // (every weight is >= 1; a total of 2^63 or more arrives here as a negative int64)
        return fail(IHG_ERR_INVALID, "ihg_sample_pool_weighted: need n_items <= total < 2^63, got total = %lld and n_items = %lld", (long long)total, (long long)n_items);
    if (n_lists < 0 || max_list_len < 0)
        return fail(IHG_ERR_INVALID, "ihg_sample_pool_weighted: need n_lists >= 0 and max_list_len >= 0, got n_lists = %lld and max_list_len = %lld", (long long)n_lists,
                    (long long)max_list_len);
    if (max_list_len > n_items - m)                                      // (the row with the longest list would have fewer than m values to find: its loop would not end)
        return fail(IHG_ERR_INVALID, "ihg_sample_pool_weighted: need m + max_list_len <= n_items, got m = %d, max_list_len = %lld and n_items = %lld", m,
                    (long long)max_list_len, (long long)n_items);
    if (n_rows == 0) return IHG_OK;
    if (cum == nullptr || out == nullptr || (n_lists > 0 && (list_of_row == nullptr || list_ptr == nullptr || list_items == nullptr)))
        return fail(IHG_ERR_INVALID, "ihg_sample_pool_weighted: null pointer");
    const int grid = static_cast<int>(std::min<int64_t>(n_rows, static_cast<int64_t>(kMaxBlocks) * kWavesPerBlock));
    hipLaunchKernelGGL(sample_pool_weighted_kernel, dim3(grid), dim3(kWave), 0, static_cast<hipStream_t>(stream), seed, counter, n_rows, n_items, static_cast<int>(m), cum,
                       static_cast<uint64_t>(total), n_lists > 0 ? list_of_row : nullptr, n_lists, list_ptr, list_items, out);
    return check_launch("ihg_sample_pool_weighted");
}

int ihg_device_batch(uint64_t seed, uint64_t counter, const int64_t* pos_triples, const int64_t* edge_ids, int64_t n, const int32_t* pair_of_edge,
                     const int64_t* neg_ptr, const int32_t* neg_items, int64_t n_items, int32_t k_rand, int32_t k_logged, int64_t* pack, ihg_stream_t stream) {
    if (n < 0 || n_items <= 0 || k_rand < 0 || k_logged < 0 || k_rand > kSampleMax || k_logged > kSampleMax || k_rand + k_logged < 1 || k_rand + k_logged > kSampleMax ||
        k_rand + k_logged > n_items)
        return fail(IHG_ERR_INVALID, "ihg_device_batch: need k_rand >= 0, k_logged >= 0 and 1 <= k_rand + k_logged <= min(%d, n_items)", kSampleMax);
    if (n == 0) return IHG_OK;                                           // (an empty batch has nothing to point at)
    if (pos_triples == nullptr || edge_ids == nullptr || pack == nullptr) return fail(IHG_ERR_INVALID, "ihg_device_batch: null pointer");
    if (k_logged > 0 && (pair_of_edge == nullptr || neg_ptr == nullptr || neg_items == nullptr))
        return fail(IHG_ERR_INVALID, "ihg_device_batch: k_logged > 0 needs the lists of logged negatives (pair_of_edge, neg_ptr, neg_items)");
    const int grid = static_cast<int>(std::min<int64_t>((n + kBlockThreads - 1) / kBlockThreads, kMaxBlocks));
    hipLaunchKernelGGL(device_batch_kernel, dim3(grid), dim3(kBlockThreads), 0, static_cast<hipStream_t>(stream), seed, counter, pos_triples, edge_ids, n, pair_of_edge,
                       neg_ptr, neg_items, n_items, k_rand, k_logged, pack);
    return check_launch("ihg_device_batch");
}


// layers[l] for l >= 1 (and for l == 0 without layer0_rows) are plain [N, ld] matrices; with layer0_rows the three node types of layer 0 start at their own addresses
static LayerPtrs layer_ptrs(const float* const* layers, int32_t n_layers, int64_t ld, const float* const* layer0_rows, int64_t ld0, const int64_t* type_begin) {
    LayerPtrs lp{};
    for (int l = 0; l < n_layers; ++l) {
        for (int t = 0; t < 3; ++t) lp.x[l][t] = layers[l];
        lp.ld[l] = ld;
    }
    if (layer0_rows != nullptr) {
        const TypedRows t0 = typed_rows(layer0_rows, type_begin, ld0);
        for (int t = 0; t < 3; ++t) lp.x[0][t] = t0.p[t];
        lp.ld[0] = ld0;
    }
    return lp;
}

// The one argument check of the six HEM entry points, in the name (`what`) of the one that was called.  IHG_OK = go on: an empty batch returns after it, the buffers are looked at last.
static int hem_check(const char* what, const float* const* layers, int32_t n_layers, int64_t ld, int32_t dim, const float* const* layer0_rows, int64_t ld0,
                     const int64_t* type_begin, int64_t batch) {
    if (n_layers < 1 || n_layers > 8) return fail(IHG_ERR_INVALID, "%s: 1..8 layer outputs supported, got %d", what, n_layers);
    if (ld < dim || dim <= 0 || batch < 0 || layers == nullptr) return fail(IHG_ERR_INVALID, "%s: bad size", what);
    if (layer0_rows != nullptr && (type_begin == nullptr || ld0 < dim)) return fail(IHG_ERR_INVALID, "%s: type ranges / row stride of layer 0 missing", what);
    for (int l = layer0_rows != nullptr ? 1 : 0; l < n_layers; ++l)      // (slot 0 is not read when layer 0 is typed)
        if (layers[l] == nullptr) return fail(IHG_ERR_INVALID, "%s: null layer pointer", what);
    return IHG_OK;
}

static int hem_score_fwd(const char* what, const float* const* layers, int32_t n_layers, int64_t ld, int32_t dim, const float* const* layer0_rows, int64_t ld0,
                         const int64_t* type_begin, const int64_t* rows, const int64_t* rows_upper, const int64_t* items, const float* bias, float lambda_muq,
                         float* scores, int64_t batch, ihg_stream_t stream) {
    if (int rc = hem_check(what, layers, n_layers, ld, dim, layer0_rows, ld0, type_begin, batch)) return rc;
    if (batch == 0) return IHG_OK;
    if (rows == nullptr || items == nullptr || bias == nullptr || scores == nullptr) return fail(IHG_ERR_INVALID, "%s: null pointer", what);
    const LayerPtrs lp = layer_ptrs(layers, n_layers, ld, layer0_rows, ld0, type_begin);
    hipLaunchKernelGGL(hem_score_fwd_kernel, dim3(grid_for_waves(batch)), dim3(kBlockThreads), 0, static_cast<hipStream_t>(stream), lp, n_layers, dim,
                       rows, items, bias, lambda_muq, scores, batch, rows_upper);
    return check_launch(what);
}

static int hem_score_bwd(const char* what, const float* const* layers, int32_t n_layers, int64_t ld, int32_t dim, const float* const* layer0_rows, int64_t ld0,
                         const int64_t* type_begin, const int64_t* rows, const int64_t* rows_upper, const float* dscores, const float* grad_scale_device,
                         float grad_scale, float lambda_muq, float* rowgrad, int64_t ld_rowgrad, int64_t batch, ihg_stream_t stream) {
    if (int rc = hem_check(what, layers, n_layers, ld, dim, layer0_rows, ld0, type_begin, batch)) return rc;
    if (batch == 0) return IHG_OK;
    if (rows == nullptr || dscores == nullptr || rowgrad == nullptr || ld_rowgrad < static_cast<int64_t>(n_layers) * dim)
        return fail(IHG_ERR_INVALID, "%s: null pointer or short row stride", what);
    const LayerPtrs lp = layer_ptrs(layers, n_layers, ld, layer0_rows, ld0, type_begin);
    hipLaunchKernelGGL(hem_score_bwd_kernel, dim3(grid_for_waves(batch)), dim3(kBlockThreads), 0, static_cast<hipStream_t>(stream), lp, n_layers, dim,
                       rows, dscores, grad_scale, lambda_muq, rowgrad, ld_rowgrad, batch, grad_scale_device, rows_upper);
    return check_launch(what);
}

int ihg_hem_score_fwd(const float* const* layers, int32_t n_layers, int64_t ld, int32_t dim, const int64_t* rows, const int64_t* items,
                      const float* bias, float lambda_muq, float* scores, int64_t batch, ihg_stream_t stream) {
    return hem_score_fwd("ihg_hem_score_fwd", layers, n_layers, ld, dim, nullptr, 0, nullptr, rows, nullptr, items, bias, lambda_muq, scores, batch, stream);
}

int ihg_hem_score_bwd(const float* const* layers, int32_t n_layers, int64_t ld, int32_t dim, const int64_t* rows, const float* dscores,
                      float grad_scale, float lambda_muq, float* rowgrad, int64_t ld_rowgrad, int64_t batch, ihg_stream_t stream) {
    return hem_score_bwd("ihg_hem_score_bwd", layers, n_layers, ld, dim, nullptr, 0, nullptr, rows, nullptr, dscores, nullptr, grad_scale, lambda_muq, rowgrad, ld_rowgrad, batch,
                         stream);
}

int ihg_hem_score_fwd_typed0(const float* const* layers, int32_t n_layers, int64_t ld, int32_t dim, const float* const* layer0_rows, int64_t ld0,
                             const int64_t* type_begin, const int64_t* rows, const int64_t* rows_upper, const int64_t* items, const float* bias, float lambda_muq,
                             float* scores, int64_t batch, ihg_stream_t stream) {
    return hem_score_fwd("ihg_hem_score_fwd_typed0", layers, n_layers, ld, dim, layer0_rows, ld0, type_begin, rows, rows_upper, items, bias, lambda_muq, scores, batch, stream);
}

int ihg_hem_score_bwd_typed0(const float* const* layers, int32_t n_layers, int64_t ld, int32_t dim, const float* const* layer0_rows, int64_t ld0,
                             const int64_t* type_begin, const int64_t* rows, const int64_t* rows_upper, const float* dscores, const float* grad_scale_device,
                             float grad_scale, float lambda_muq, float* rowgrad, int64_t ld_rowgrad, int64_t batch, ihg_stream_t stream) {
    return hem_score_bwd("ihg_hem_score_bwd_typed0", layers, n_layers, ld, dim, layer0_rows, ld0, type_begin, rows, rows_upper, dscores, grad_scale_device, grad_scale, lambda_muq,
                         rowgrad, ld_rowgrad, batch, stream);
}

int ihg_hem_cosine_fwd(const float* const* layers, int32_t n_layers, int64_t ld, int32_t dim, const float* const* layer0_rows, int64_t ld0,
                       const int64_t* type_begin, const int64_t* rows, const int64_t* rows_upper, const int64_t* items, const float* bias, float lambda_muq,
                       float* scores, float* stats, int64_t batch, ihg_stream_t stream) {
    if (int rc = hem_check("ihg_hem_cosine_fwd", layers, n_layers, ld, dim, layer0_rows, ld0, type_begin, batch)) return rc;
    if (batch == 0) return IHG_OK;
    if (rows == nullptr || items == nullptr || bias == nullptr || scores == nullptr || stats == nullptr || !aligned16(stats))
        return fail(IHG_ERR_INVALID, "ihg_hem_cosine_fwd: null pointer or stats not 16-byte aligned");
    const LayerPtrs lp = layer_ptrs(layers, n_layers, ld, layer0_rows, ld0, type_begin);
    hipLaunchKernelGGL(hem_cosine_fwd_kernel, dim3(grid_for_waves(batch)), dim3(kBlockThreads), 0, static_cast<hipStream_t>(stream), lp, n_layers, dim,
                       rows, items, bias, lambda_muq, scores, reinterpret_cast<float4*>(stats), batch, rows_upper);
    return check_launch("ihg_hem_cosine_fwd");
}

int ihg_hem_cosine_bwd(const float* const* layers, int32_t n_layers, int64_t ld, int32_t dim, const float* const* layer0_rows, int64_t ld0,
                       const int64_t* type_begin, const int64_t* rows, const int64_t* rows_upper, const float* dscores, const float* stats,
                       const float* grad_scale_device, float grad_scale, float lambda_muq, float* rowgrad, int64_t ld_rowgrad, int64_t batch, ihg_stream_t stream) {
    if (int rc = hem_check("ihg_hem_cosine_bwd", layers, n_layers, ld, dim, layer0_rows, ld0, type_begin, batch)) return rc;
    if (batch == 0) return IHG_OK;
    if (rows == nullptr || dscores == nullptr || stats == nullptr || !aligned16(stats) || rowgrad == nullptr || ld_rowgrad < static_cast<int64_t>(n_layers) * dim)
        return fail(IHG_ERR_INVALID, "ihg_hem_cosine_bwd: null pointer, stats not 16-byte aligned or short row stride");
    const LayerPtrs lp = layer_ptrs(layers, n_layers, ld, layer0_rows, ld0, type_begin);
    hipLaunchKernelGGL(hem_cosine_bwd_kernel, dim3(grid_for_waves(batch)), dim3(kBlockThreads), 0, static_cast<hipStream_t>(stream), lp, n_layers, dim,
                       rows, dscores, reinterpret_cast<const float4*>(stats), grad_scale, lambda_muq, rowgrad, ld_rowgrad, batch, grad_scale_device, rows_upper);
    return check_launch("ihg_hem_cosine_bwd");
}

int ihg_bce_with_logits(const float* scores, const float* labels, int64_t n, float* loss, float* dscores, ihg_stream_t stream) {
    if (n <= 0 || n > (1 << 24) || scores == nullptr || labels == nullptr || loss == nullptr || dscores == nullptr)
        return fail(IHG_ERR_INVALID, "ihg_bce_with_logits: bad argument");
    hipLaunchKernelGGL(bce_with_logits_kernel, dim3(1), dim3(kScatterThreads), 0, static_cast<hipStream_t>(stream), scores, labels, static_cast<int>(n), loss, dscores);
    return check_launch("ihg_bce_with_logits");
}

int ihg_ranking_loss(const float* scores, int64_t positives, int32_t k, int32_t kind, float* loss, float* dscores, ihg_stream_t stream) {
    if (scores == nullptr || loss == nullptr || dscores == nullptr) return fail(IHG_ERR_INVALID, "ihg_ranking_loss: null pointer");
    if (positives < 1 || k < 1) return fail(IHG_ERR_INVALID, "ihg_ranking_loss: need positives >= 1 and k >= 1, got %lld and %d", (long long)positives, k);
    if (kind != kLossBpr && kind != kLossSoftmax) return fail(IHG_ERR_INVALID, "ihg_ranking_loss: kind is IHG_LOSS_BPR (1) or IHG_LOSS_SOFTMAX (2), got %d", kind);
    if (positives > INT32_MAX / (static_cast<int64_t>(k) + 1))
        return fail(IHG_ERR_INVALID, "ihg_ranking_loss: positives * (1 + k) = %lld * %lld is beyond INT32_MAX scores", (long long)positives, (long long)k + 1);
    const auto kernel = kind == kLossBpr ? ranking_loss_kernel<kLossBpr> : ranking_loss_kernel<kLossSoftmax>;
    hipLaunchKernelGGL(kernel, dim3(1), dim3(kScatterThreads), 0, static_cast<hipStream_t>(stream), scores, static_cast<int>(positives), static_cast<int>(k), loss, dscores);
    return check_launch("ihg_ranking_loss");
}

int ihg_hard_negative_loss(const float* scores, int64_t positives, int32_t pool, int32_t keep, int32_t kind, float* loss, float* dscores, int32_t* selected,
                           ihg_stream_t stream) {
    if (scores == nullptr || loss == nullptr || dscores == nullptr || selected == nullptr) return fail(IHG_ERR_INVALID, "ihg_hard_negative_loss: null pointer");
    if (positives < 1) return fail(IHG_ERR_INVALID, "ihg_hard_negative_loss: need positives >= 1, got %lld", (long long)positives);
    if (keep < 1 || keep > pool || pool > kPoolMax)
        return fail(IHG_ERR_INVALID, "ihg_hard_negative_loss: need 1 <= keep <= pool <= %d, got keep = %d and pool = %d", kPoolMax, keep, pool);
    if (kind != kLossBce && kind != kLossBpr && kind != kLossSoftmax)
        return fail(IHG_ERR_INVALID, "ihg_hard_negative_loss: kind is IHG_LOSS_BCE (0), IHG_LOSS_BPR (1) or IHG_LOSS_SOFTMAX (2), got %d", kind);
    if (positives > INT32_MAX / (static_cast<int64_t>(pool) + 1))
        return fail(IHG_ERR_INVALID, "ihg_hard_negative_loss: positives * (1 + pool) = %lld * %lld is beyond INT32_MAX scores", (long long)positives, (long long)pool + 1);
    const auto kernel = kind == kLossBce ? hard_negative_loss_kernel<kLossBce> : kind == kLossBpr ? hard_negative_loss_kernel<kLossBpr> : hard_negative_loss_kernel<kLossSoftmax>;
    hipLaunchKernelGGL(kernel, dim3(1), dim3(kScatterThreads), 0, static_cast<hipStream_t>(stream), scores, static_cast<int>(positives), static_cast<int>(pool),
                       static_cast<int>(keep), loss, dscores, selected);
    return check_launch("ihg_hard_negative_loss");
}


int64_t ihg_batch_scatter_workspace_bytes(int64_t n_rows) {
    return (n_rows < 0 || n_rows > kScatterMaxWide) ? -1 : 0;
}

int32_t ihg_batch_scatter_max_rows(void) { return kScatterMaxWide; }

int ihg_batch_scatter_add(const float* rowgrad, int64_t ld_rowgrad, int32_t width, const int64_t* rows, int64_t n_rows, float* dense,
                          int64_t ld_dense, int32_t block_width, int64_t block_stride, float* tail, int64_t tail_row_offset,
                          int64_t tail_rows, ihg_stream_t stream) {
    if (n_rows < 0 || n_rows > kScatterMaxWide) return fail(IHG_ERR_INVALID, "ihg_batch_scatter_add: 0..%d rows supported, got %lld", kScatterMaxWide, (long long)n_rows);
    if (width <= 0 || ld_rowgrad < width || block_width <= 0 || ld_dense < block_width) return fail(IHG_ERR_INVALID, "ihg_batch_scatter_add: bad width / stride");
    if (n_rows == 0) return IHG_OK;
    if (rowgrad == nullptr || rows == nullptr || dense == nullptr) return fail(IHG_ERR_INVALID, "ihg_batch_scatter_add: null pointer");
    const dim3 grid(grid_for_waves(n_rows), 1);              // one block: any two rows may share a destination
    if (n_rows > kScatterMax)
        hipLaunchKernelGGL((batch_scatter_kernel<false, kScatterMaxWide>), grid, dim3(kBlockThreads), 0, static_cast<hipStream_t>(stream),
                           const_cast<float*>(rowgrad), ld_rowgrad, width, rows, static_cast<int>(n_rows), dense, ld_dense, block_width, block_stride, tail,
                           tail_row_offset, tail_rows, static_cast<int32_t*>(nullptr), static_cast<int>(n_rows));
    else
        hipLaunchKernelGGL((batch_scatter_kernel<false>), grid, dim3(kBlockThreads), 0, static_cast<hipStream_t>(stream),
                           const_cast<float*>(rowgrad), ld_rowgrad, width, rows, static_cast<int>(n_rows), dense, ld_dense, block_width, block_stride, tail,
                           tail_row_offset, tail_rows, static_cast<int32_t*>(nullptr), static_cast<int>(n_rows));
    return check_launch("ihg_batch_scatter_add");
}

int ihg_batch_combine(float* rowgrad, int64_t ld_rowgrad, int32_t width, const int64_t* rows, int64_t n_rows, int64_t disjoint_block_rows,
                      int32_t* leader, ihg_stream_t stream) {
    if (n_rows < 0 || n_rows > kScatterMaxWide) return fail(IHG_ERR_INVALID, "ihg_batch_combine: 0..%d rows supported, got %lld", kScatterMaxWide, (long long)n_rows);
    if (width <= 0 || ld_rowgrad < width) return fail(IHG_ERR_INVALID, "ihg_batch_combine: bad width / stride");
    if (n_rows == 0) return IHG_OK;
    if (rowgrad == nullptr || rows == nullptr || leader == nullptr) return fail(IHG_ERR_INVALID, "ihg_batch_combine: null pointer");
    if (disjoint_block_rows <= 0 || disjoint_block_rows > n_rows) disjoint_block_rows = n_rows;
    const int n_blocks = static_cast<int>((n_rows + disjoint_block_rows - 1) / disjoint_block_rows);
    const dim3 grid(grid_for_waves(disjoint_block_rows), n_blocks);      // a workgroup works inside one block and holds that block's ids only
    if (disjoint_block_rows > kScatterMax)
        hipLaunchKernelGGL((batch_scatter_kernel<true, kScatterMaxWide>), grid, dim3(kBlockThreads), 0, static_cast<hipStream_t>(stream), rowgrad,
                           ld_rowgrad, width, rows, static_cast<int>(n_rows), static_cast<float*>(nullptr), int64_t{0}, 1, int64_t{0},
                           static_cast<float*>(nullptr), int64_t{0}, int64_t{0}, leader, static_cast<int>(disjoint_block_rows));
    else
        hipLaunchKernelGGL((batch_scatter_kernel<true>), grid, dim3(kBlockThreads), 0, static_cast<hipStream_t>(stream), rowgrad,
                           ld_rowgrad, width, rows, static_cast<int>(n_rows), static_cast<float*>(nullptr), int64_t{0}, 1, int64_t{0},
                           static_cast<float*>(nullptr), int64_t{0}, int64_t{0}, leader, static_cast<int>(disjoint_block_rows));
    return check_launch("ihg_batch_combine");
}

int ihg_batch_rows_add(const float* src, int64_t ld_src, int32_t width, const int64_t* rows, const int32_t* leader, int64_t n_rows, float* dense,
                       int64_t ld_dense, float* tail, int64_t tail_row_offset, int64_t tail_rows, ihg_stream_t stream) {
    if (n_rows < 0 || width <= 0 || ld_src < width) return fail(IHG_ERR_INVALID, "ihg_batch_rows_add: bad size");
    if (n_rows == 0) return IHG_OK;
    if (src == nullptr || rows == nullptr || leader == nullptr || (dense == nullptr && tail == nullptr) || (dense != nullptr && ld_dense < width))
        return fail(IHG_ERR_INVALID, "ihg_batch_rows_add: null pointer or short row stride");
    hipLaunchKernelGGL(batch_rows_add_kernel<false>, dim3(grid_for_waves(n_rows)), dim3(kBlockThreads), 0, static_cast<hipStream_t>(stream), src, ld_src, width,
                       rows, leader, static_cast<int>(n_rows), typed_rows_out(dense), int64_t{0}, int64_t{0}, ld_dense, tail, tail_row_offset, tail_rows);
    return check_launch("ihg_batch_rows_add");
}

int ihg_batch_rows_put(const float* src, int64_t ld_src, int32_t width, const int64_t* rows, const int32_t* leader, int64_t n_rows, float* const* dense_rows,
                       int64_t ld_dense, const int64_t* type_begin, int32_t assign, ihg_stream_t stream) {
    if (n_rows < 0 || width <= 0 || ld_src < width || ld_dense < width) return fail(IHG_ERR_INVALID, "ihg_batch_rows_put: bad size");
    if (n_rows == 0) return IHG_OK;
    if (src == nullptr || rows == nullptr || leader == nullptr || dense_rows == nullptr || type_begin == nullptr) return fail(IHG_ERR_INVALID, "ihg_batch_rows_put: null pointer");
    const TypedRowsOut dense = typed_rows_out(dense_rows, type_begin, ld_dense);
    if (assign)
        hipLaunchKernelGGL(batch_rows_add_kernel<true>, dim3(grid_for_waves(n_rows)), dim3(kBlockThreads), 0, static_cast<hipStream_t>(stream), src, ld_src, width, rows, leader,
                           static_cast<int>(n_rows), dense, type_begin[1], type_begin[2], ld_dense, static_cast<float*>(nullptr), int64_t{0}, int64_t{0});
    else
        hipLaunchKernelGGL(batch_rows_add_kernel<false>, dim3(grid_for_waves(n_rows)), dim3(kBlockThreads), 0, static_cast<hipStream_t>(stream), src, ld_src, width, rows, leader,
                           static_cast<int>(n_rows), dense, type_begin[1], type_begin[2], ld_dense, static_cast<float*>(nullptr), int64_t{0}, int64_t{0});
    return check_launch("ihg_batch_rows_put");
}

int ihg_zero_floats(float* p, int64_t n, ihg_stream_t stream) {
    if (n < 0 || (n > 0 && p == nullptr)) return fail(IHG_ERR_INVALID, "ihg_zero_floats: bad argument");
    launch_zero_floats(p, n, static_cast<hipStream_t>(stream));
    return check_launch("ihg_zero_floats");
}

int ihg_mark_rows(const int64_t* rows64, const int32_t* rows32, int64_t n, uint8_t* mask, int32_t value, ihg_stream_t stream) {
    if (n < 0 || (n > 0 && (mask == nullptr || (rows64 == nullptr) == (rows32 == nullptr)))) return fail(IHG_ERR_INVALID, "ihg_mark_rows: one of rows64 / rows32 and a mask");
    if (n == 0) return IHG_OK;
    const int grid = static_cast<int>(std::min<int64_t>((n + kBlockThreads - 1) / kBlockThreads, kMaxBlocks));
    hipLaunchKernelGGL(mark_rows_kernel, dim3(grid), dim3(kBlockThreads), 0, static_cast<hipStream_t>(stream), rows64, rows32, n, mask, static_cast<uint8_t>(value));
    return check_launch("ihg_mark_rows");
}

int ihg_zero_rows(float* base, int64_t ld, int32_t dim, const int64_t* rows, int64_t n, ihg_stream_t stream) {
    if (n < 0 || dim <= 0 || ld < dim || (n > 0 && (base == nullptr || rows == nullptr))) return fail(IHG_ERR_INVALID, "ihg_zero_rows: bad argument");
    if (n == 0) return IHG_OK;
    hipLaunchKernelGGL(zero_rows_kernel, dim3(grid_for_waves(n)), dim3(kBlockThreads), 0, static_cast<hipStream_t>(stream), base, ld, dim, rows, n);
    return check_launch("ihg_zero_rows");
}

int ihg_batch_node_rows(const int64_t* users, const int64_t* queries, const int64_t* items, int64_t batch, int64_t query_row0, int64_t item_row0, int64_t* rows,
                        int32_t* rows32, ihg_stream_t stream) {
    if (batch < 0 || (batch > 0 && (users == nullptr || queries == nullptr || items == nullptr || rows == nullptr))) return fail(IHG_ERR_INVALID, "ihg_batch_node_rows: bad argument");
    if (batch == 0) return IHG_OK;
    const int grid = static_cast<int>(std::min<int64_t>((3 * batch + kBlockThreads - 1) / kBlockThreads, kMaxBlocks));
    hipLaunchKernelGGL(batch_node_rows_kernel, dim3(grid), dim3(kBlockThreads), 0, static_cast<hipStream_t>(stream), users, queries, items, batch, query_row0, item_row0, rows, rows32);
    return check_launch("ihg_batch_node_rows");
}

static int adam_launch(const char* what, const ihg_adam_tensor* tensors, int32_t n_tensors, float beta1, float beta2, float eps, float weight_decay, float step_size,
                       float bias2_sqrt, const float* scalars, const float* clip, ihg_stream_t stream) {
    for (int t = 0; t < n_tensors; ++t) {                    // every tensor is checked before the first launch: a refused call has updated nothing
        const ihg_adam_tensor& a = tensors[t];
        if (a.count < 0 || (a.count > 0 && (a.param == nullptr || a.grad == nullptr || a.exp_avg == nullptr || a.exp_avg_sq == nullptr)))
            return fail(IHG_ERR_INVALID, "%s: tensor %d has a null pointer or a negative count", what, t);
    }
    bool launched = false;
    for (int t = 0; t < n_tensors;) {                        // one launch per kAdamMaxTensors NON-EMPTY tensors; t is the only cursor
        AdamTable tab{};
        int64_t chunks = 0;
        int used = 0;
        for (; t < n_tensors && used < kAdamMaxTensors; ++t) {
            const ihg_adam_tensor& a = tensors[t];
            if (a.count == 0) continue;
            tab.param[used] = a.param; tab.grad[used] = a.grad; tab.exp_avg[used] = a.exp_avg; tab.exp_avg_sq[used] = a.exp_avg_sq;
            tab.count[used] = a.count;
            tab.chunk_begin[used] = chunks;
            chunks += (a.count + kAdamChunk - 1) / kAdamChunk;
            ++used;
        }
        tab.chunk_begin[used] = chunks;
        tab.n_tensors = used;
        if (used == 0) continue;
        const int grid = static_cast<int>(std::min<int64_t>(chunks, 256 * 16));
        if (clip != nullptr)
            hipLaunchKernelGGL(adam_kernel<true>, dim3(grid), dim3(kBlockThreads), 0, static_cast<hipStream_t>(stream), tab, beta1, beta2, eps, weight_decay,
                               step_size, bias2_sqrt, scalars, clip);
        else
            hipLaunchKernelGGL(adam_kernel<false>, dim3(grid), dim3(kBlockThreads), 0, static_cast<hipStream_t>(stream), tab, beta1, beta2, eps, weight_decay,
                               step_size, bias2_sqrt, scalars, clip);
        launched = true;
    }
    return launched ? check_launch(what) : IHG_OK;           // (only empty tensors: nothing was launched, the runtime is not asked)
}

int ihg_adam_step(const ihg_adam_tensor* tensors, int32_t n_tensors, float lr, float beta1, float beta2, float eps, float weight_decay,
                  int64_t step, ihg_stream_t stream) {
    if (n_tensors < 0 || (n_tensors > 0 && tensors == nullptr) || step < 1) return fail(IHG_ERR_INVALID, "ihg_adam_step: bad argument");
    const double bias1 = 1.0 - std::pow(static_cast<double>(beta1), static_cast<double>(step));
    const double bias2 = 1.0 - std::pow(static_cast<double>(beta2), static_cast<double>(step));
    return adam_launch("ihg_adam_step", tensors, n_tensors, beta1, beta2, eps, weight_decay, static_cast<float>(static_cast<double>(lr) / bias1),
                       static_cast<float>(std::sqrt(bias2)), nullptr, nullptr, stream);
}

int ihg_adam_step_device_scalars(const ihg_adam_tensor* tensors, int32_t n_tensors, float beta1, float beta2, float eps, float weight_decay,
                                 const float* step_scalars, ihg_stream_t stream) {
    if (n_tensors < 0 || (n_tensors > 0 && tensors == nullptr) || step_scalars == nullptr) return fail(IHG_ERR_INVALID, "ihg_adam_step_device_scalars: bad argument");
    return adam_launch("ihg_adam_step_device_scalars", tensors, n_tensors, beta1, beta2, eps, weight_decay, 0.f, 1.f, step_scalars, nullptr, stream);
}

int ihg_adam_step_clipped(const ihg_adam_tensor* tensors, int32_t n_tensors, float lr, float beta1, float beta2, float eps, float weight_decay,
                          int64_t step, const float* clip, ihg_stream_t stream) {
    if (n_tensors < 0 || (n_tensors > 0 && tensors == nullptr) || step < 1 || clip == nullptr) return fail(IHG_ERR_INVALID, "ihg_adam_step_clipped: bad argument");
    const double bias1 = 1.0 - std::pow(static_cast<double>(beta1), static_cast<double>(step));
    const double bias2 = 1.0 - std::pow(static_cast<double>(beta2), static_cast<double>(step));
    return adam_launch("ihg_adam_step_clipped", tensors, n_tensors, beta1, beta2, eps, weight_decay, static_cast<float>(static_cast<double>(lr) / bias1),
                       static_cast<float>(std::sqrt(bias2)), nullptr, clip, stream);
}

int ihg_adam_step_clipped_device_scalars(const ihg_adam_tensor* tensors, int32_t n_tensors, float beta1, float beta2, float eps, float weight_decay,
                                         const float* step_scalars, const float* clip, ihg_stream_t stream) {
    if (n_tensors < 0 || (n_tensors > 0 && tensors == nullptr) || step_scalars == nullptr || clip == nullptr)
        return fail(IHG_ERR_INVALID, "ihg_adam_step_clipped_device_scalars: bad argument");
    return adam_launch("ihg_adam_step_clipped_device_scalars", tensors, n_tensors, beta1, beta2, eps, weight_decay, 0.f, 1.f, step_scalars, clip, stream);
}

// chunks of the non-empty tensors, or -1 for a bad table (a negative count, a gradient missing where count > 0)
static int64_t grad_sqnorm_chunks(const char* what, const ihg_adam_tensor* tensors, int32_t n_tensors) {
    if (n_tensors < 0 || (n_tensors > 0 && tensors == nullptr)) {
        fail(IHG_ERR_INVALID, "%s: bad argument", what);
        return -1;
    }
    int64_t chunks = 0;
    for (int t = 0; t < n_tensors; ++t) {
        if (tensors[t].count < 0 || (tensors[t].count > 0 && tensors[t].grad == nullptr)) {
            fail(IHG_ERR_INVALID, "%s: tensor %d has a null gradient or a negative count", what, t);
            return -1;
        }
        chunks += (tensors[t].count + kAdamChunk - 1) / kAdamChunk;
    }
    return chunks;
}

int64_t ihg_grad_sqnorm_workspace_bytes(const ihg_adam_tensor* tensors, int32_t n_tensors) {
    const int64_t chunks = grad_sqnorm_chunks("ihg_grad_sqnorm_workspace_bytes", tensors, n_tensors);
    return chunks < 0 ? -1 : chunks * static_cast<int64_t>(sizeof(double));
}

int ihg_grad_sqnorm(const ihg_adam_tensor* tensors, int32_t n_tensors, void* workspace, int64_t workspace_bytes, double* sum, ihg_stream_t stream) {
    const int64_t total = grad_sqnorm_chunks("ihg_grad_sqnorm", tensors, n_tensors);
    if (total < 0) return IHG_ERR_INVALID;
    if (sum == nullptr || (reinterpret_cast<uintptr_t>(sum) & 7) != 0) return fail(IHG_ERR_INVALID, "ihg_grad_sqnorm: sum is null or not 8-byte aligned");
    if (total > 0 && (workspace == nullptr || (reinterpret_cast<uintptr_t>(workspace) & 7) != 0))
        return fail(IHG_ERR_INVALID, "ihg_grad_sqnorm: workspace is null or not 8-byte aligned");
    if (workspace_bytes < total * static_cast<int64_t>(sizeof(double)))
        return fail(IHG_ERR_WORKSPACE, "ihg_grad_sqnorm: workspace too small (%lld bytes, %lld needed)", (long long)workspace_bytes, (long long)(total * sizeof(double)));
    double* partials = static_cast<double*>(workspace);
    int64_t done = 0;                                        // chunks of the launches so far: the numbering goes on through the workspace
    for (int t = 0; t < n_tensors;) {
        GradNormTable tab{};
        int64_t chunks = 0;
        int used = 0;
        for (; t < n_tensors && used < kAdamMaxTensors; ++t) {
            const ihg_adam_tensor& a = tensors[t];
            if (a.count == 0) continue;
            tab.grad[used] = a.grad;
            tab.count[used] = a.count;
            tab.chunk_begin[used] = chunks;
            chunks += (a.count + kAdamChunk - 1) / kAdamChunk;
            ++used;
        }
        tab.chunk_begin[used] = chunks;
        tab.n_tensors = used;
        if (used == 0) continue;
        const int grid = static_cast<int>(std::min<int64_t>(chunks, 256 * 16));
        hipLaunchKernelGGL(grad_sqnorm_partial_kernel, dim3(grid), dim3(kBlockThreads), 0, static_cast<hipStream_t>(stream), tab, partials + done);
        done += chunks;
    }
    hipLaunchKernelGGL(grad_sqnorm_finish_kernel, dim3(1), dim3(kBlockThreads), 0, static_cast<hipStream_t>(stream), partials, done, sum);      // (no chunks: sum = 0)
    return check_launch("ihg_grad_sqnorm");
}

int ihg_clip_record(const double* sum, float max_norm, float* clip, float* stats, ihg_stream_t stream) {
    if (sum == nullptr || clip == nullptr || (reinterpret_cast<uintptr_t>(sum) & 7) != 0) return fail(IHG_ERR_INVALID, "ihg_clip_record: null pointer or unaligned sum");
    if (!(max_norm >= 0.f)) return fail(IHG_ERR_INVALID, "ihg_clip_record: max_norm must be >= 0 (inf allowed), got %g", static_cast<double>(max_norm));
    hipLaunchKernelGGL(clip_record_kernel, dim3(1), dim3(kWave), 0, static_cast<hipStream_t>(stream), sum, max_norm, clip, stats);
    return check_launch("ihg_clip_record");
}
}  // extern "C"
