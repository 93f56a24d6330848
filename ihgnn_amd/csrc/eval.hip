// eval.hip - evaluation scoring: HEM scores of many (user, query) pairs against EVERY item with a running top-k per
// pair, on the matrix cores, without materialising the [pairs, items] score matrix.
//
// Reference: per search log, RawGnn.forward(u * ones(I), q * ones(I), None) (Models/RawGnn.py:124-137) broadcasts one user row and
// one query row to [I, D], HemPredictionLayer scores them (Models/PredictionLayers.py:35-43) and Metrics.calculate_on_all_items
// (Helpers/Metrics.py:60-61) sorts all I scores and keeps ten.  Here a workgroup owns a block of 32 pairs - their mixed rows
// m = lam * F[q] + (1 - lam) * F[u] sit in LDS for the whole kernel - and its four waves stream disjoint runs of item rows as the
// A operand of v_mfma_f32_32x32x2_f32 (exact fp32): the 32 x 32 result tile has the PAIR on the lane (column) and 16 items in the
// lane's accumulator registers, so every lane keeps the running top-k of "its" pair over the items it has seen in registers, with
// no cross-lane traffic in the loop.  The partial lists (2 lane halves x 4 waves x item slices per pair) are merged by a second,
// tiny kernel.  Order: higher score first, equal scores by lower item index (= a stable descending sort; the reference's
// torch.sort is unstable on ties).
// Entry points: ihg_score_topk / _cosine (k <= 10), ihg_score_topk_deep (k <= 128, in passes), ihg_search_topk (external query rows, no user, a candidate mask) and
// ihg_search_topk_excluding (a run of excluded items per pair) - one kernel family by template flags, one host path at the end of this file.
#include "ranking.hpp"

namespace {

// ------------------------------------------------------------------------------------------------
// Arithmetic: fp32 through TWO fp16 terms (split_arith.hip has the scheme and its error analysis): every item row and every mixed row is multiplied by the power of
// two that brings its largest magnitude to [2^13, 2^14), x = hi + lo with hi = fp16(x), lo = fp16(x - hi), and a product is hi lo + lo hi + hi hi on
// v_mfma_f32_32x32x16_f16, fp32 accumulation; the score is the accumulator times the two inverse scales (exact: powers of two) plus the bias.  Unlike the training
// kernels nothing is split inside the hot loop: the item rows are split ONCE per call into MFMA-fragment order (score_prepare_kernel: 1 KB per (tile, k-step, plane), a
// fully coalesced wave load), the mixed rows of a pair block once into LDS - the loop is loads, LDS reads and MFMAs.  A workgroup owns PB x 32 pairs (PB = 2 where their
// planes fit LDS: widths up to 624) and its eight waves stream disjoint runs of item tiles: every item row is fetched once per 32 PB pairs.
// ------------------------------------------------------------------------------------------------
typedef _Float16 v8h __attribute__((ext_vector_type(8)));
typedef _Float16 v2h __attribute__((ext_vector_type(2)));
typedef unsigned v4u __attribute__((ext_vector_type(4)));

constexpr int kEvalThreads = 512;

__device__ __forceinline__ float eval_scale_up_for(float m, float& inverse) {      // 2^(13 - floor(log2 m)) and its inverse (exponent clamped; split_arith.hip scale_up_for)
    int e = static_cast<int>((__float_as_uint(m) >> 23) & 0xffu);
    e = e < 27 ? 27 : (e > 227 ? 227 : e);
    inverse = __uint_as_float(static_cast<unsigned>(e - 13) << 23);
    return __uint_as_float(static_cast<unsigned>(267 - e) << 23);
}
__device__ __forceinline__ void eval_split8(const float (&x)[8], v4u& hi, v4u& lo) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const v2h h = v2h{static_cast<_Float16>(x[2 * i]), static_cast<_Float16>(x[2 * i + 1])};
        const v2h l = v2h{static_cast<_Float16>(x[2 * i] - static_cast<float>(h[0])), static_cast<_Float16>(x[2 * i + 1] - static_cast<float>(h[1]))};
        hi[i] = __builtin_bit_cast(unsigned, h);
        lo[i] = __builtin_bit_cast(unsigned, l);
    }
}

// Item rows -> frag[tile][ks][plane][lane][8 x fp16] (tile = 32 items, ks = 16 columns; lane = 32 (column half of the k-step) + item % 32: the A fragment of
// v_mfma_f32_32x32x16_f16), aux[item] = {inverse scale, bias}.  One wave per item row; columns past `dim` are zero.
// COSINE (Gs.Prediction.use_cosine_similarity, PredictionLayers.py:38-40): the row's sum of squares is reduced beside its largest magnitude and
// aux[item].x = inverse scale / max(||a||, 1e-8) - the hot loop of score_topk_kernel multiplies by it as it does by the plain inverse scale.
//
// What ihg_search_topk adds to the deep call (an empty struct for every other instantiation, as DeepArgs<false>): an external query row per pair, the candidate
// mask and the ranks a complete pair has, formed on the device (search_target_kernel) where the mask decides it.
template <bool SEARCH>
struct SearchArgs {};
template <>
struct SearchArgs<true> {
    const float* query_rows;                                                // [n_pairs, q_dim] (row stride ld_q), columns q_dim.. count as zero and are never read; null: `queries`
    int64_t ld_q;
    int q_dim;
    const uint32_t* item_mask;                                              // bit i % 32 of word i / 32: item i is a candidate; null: every item
    const int32_t* target;                                                  // min(k, candidates); EXCL: [n_pairs], min(k, the candidates of pair c that it does not exclude)
};

// What ihg_search_topk_excluding adds to the search call (an empty struct for every other instantiation): per pair a strictly ascending run of item ids that are
// never ranked for it.  A lane owns one pair per pair tile and meets that pair's items in ascending id order - within a tile (8 r4 + 4 half + x) and from tile to
// tile - so it follows the run with a cursor: the cost is that of the run, not of pairs x items.
template <bool EXCL>
struct ExclArgs {};
template <>
struct ExclArgs<true> {
    const int64_t* ptr;                                                     // [rows + 1]
    const int32_t* items;                                                   // [ptr[rows]]
    const int64_t* row;                                                     // [n_pairs]: the run of pair c, < 0: none; null: run c
};

// the cursor of one lane into the run of one pair: `next` is the run's first id not yet passed (INT_MAX: spent, or no run)
struct ExclCursor {
    const int32_t* at;
    const int32_t* end;
    int next;
    __device__ __forceinline__ void step() {
        ++at;
        next = at < end ? *at : INT_MAX;
    }
};

// SEARCH: an item outside the mask gets aux = {0, -inf} and nothing else - whatever its stale planes multiply to, its score is -inf or NaN, which ranks before no
// list entry (not even the empty (-FLT_MAX, INT_MAX)) and after no boundary: the hot loop of score_topk_kernel is the same code with or without a mask.
template <bool COSINE = false, bool SEARCH = false>
__global__ __launch_bounds__(kBlockThreads) void score_prepare_kernel(const float* __restrict__ feat, int64_t ld, int dim, int ksteps, int64_t item_row0, int64_t n_items,
                                                                      const float* __restrict__ bias, v4u* __restrict__ frag, float2* __restrict__ aux,
                                                                      [[maybe_unused]] const SearchArgs<SEARCH> search) {
    const int lane = threadIdx.x & 63;
    for (int64_t item = global_wave_id(); item < n_items; item += global_wave_count()) {
        if constexpr (SEARCH) {
            if (search.item_mask != nullptr && ((search.item_mask[item >> 5] >> (item & 31)) & 1u) == 0) {      // (wave-uniform)
                if (lane == 0) aux[item] = make_float2(0.f, -__builtin_inff());
                continue;
            }
        }
        const float* row = feat + (item_row0 + item) * ld;
        float m = 0.f;
        [[maybe_unused]] float ss = 0.f;
        for (int c = lane; c < dim; c += kWave) {
            const float v = row[c];
            m = fmaxf(m, fabsf(v));
            if constexpr (COSINE) ss += v * v;
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) m = fmaxf(m, __shfl_xor(m, off));
        float inv;
        const float sc = eval_scale_up_for(m, inv);
        if constexpr (COSINE) {
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) ss += __shfl_xor(ss, off);
            inv /= fmaxf(sqrtf(ss), kCosineEps);
        }
        if (lane == 0) aux[item] = make_float2(inv, bias[item]);
        const int64_t tile = item >> 5;
        for (int chunk = lane; chunk < 2 * ksteps; chunk += kWave) {      // eight consecutive columns
            float x[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) x[i] = 8 * chunk + i < dim ? row[8 * chunk + i] * sc : 0.f;
            v4u hi, lo;
            eval_split8(x, hi, lo);
            const int64_t base = ((tile * ksteps + (chunk >> 1)) * 2) * kWave + 32 * (chunk & 1) + (item & 31);
            frag[base] = hi;
            frag[base + kWave] = lo;
        }
    }
}

// What a pair carries from one pass of the deep top-k (k > kTopMax, ihg_score_topk_deep) to the next: `count` ranks are in the output, the last of them is the
// boundary (b_val, b_idx); `passes` counts the passes that found the pair incomplete.
struct DeepState {
    float b_val;
    int32_t b_idx;
    int32_t count;
    int32_t passes;
};

// grid (pair blocks of 32 PB pairs, item slices); 512 threads.  partial[(pair * n_lists + list) * kTopMax + p]
// DEEP (ihg_score_topk_deep): a candidate enters a lane's list only if it ranks strictly after its pair's boundary, and a workgroup whose pairs all have
// `target` ranks returns before it touches LDS or the item fragments.  The scores are those of the plain kernel, bit for bit: one expression, one item order.
template <bool DEEP>
struct DeepArgs {};
template <>
struct DeepArgs<true> {
    const DeepState* state;
    int target;                                                             // min(k, n_items): the ranks a complete pair has
};

// SEARCH (ihg_search_topk; always with DEEP): the query row of a pair may come from `search.query_rows` (zero past q_dim), users[c] < 0 names no user - the mixed
// row is the query row itself (PredictionLayers.py:34-37, user_feature is None) - and the ranks of a complete pair are read from `search.target`.
// EXCL (ihg_search_topk_excluding; always with SEARCH): search.target is per pair, and an item of the pair's run never enters the lane's list.  Its score is
// computed like every other (one expression, one item order: the scores that remain are the bits of ihg_search_topk); exclusion only gates the insert.
template <int PB, bool COSINE = false, bool DEEP = false, bool SEARCH = false, bool EXCL = false>
__global__ __launch_bounds__(kEvalThreads) void score_topk_kernel(
    const float* __restrict__ feat, int64_t ld, int dim, int ksteps, const v4u* __restrict__ frag, const float2* __restrict__ aux, int64_t n_items,
    const int64_t* __restrict__ users, const int64_t* __restrict__ queries, int64_t query_row0, float lam, int64_t n_pairs,
    float* __restrict__ part_val, int32_t* __restrict__ part_idx, [[maybe_unused]] const DeepArgs<DEEP> deep, [[maybe_unused]] const SearchArgs<SEARCH> search,
    [[maybe_unused]] const ExclArgs<EXCL> excl) {
    static_assert(DEEP || !SEARCH, "the search arguments ride on the deep passes");
    static_assert(SEARCH || !EXCL, "the exclusion lists ride on the search arguments");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];    // mixed planes: [32 PB][hi: 2 dp bytes | lo: 2 dp bytes | 16 bytes of padding], then pinv[32 PB]
    if constexpr (DEEP) {                                                   // every wave asks the same question of the same (read-only) state: no barrier
        const int64_t pr = static_cast<int64_t>(blockIdx.x) * (32 * PB) + (threadIdx.x & 63);
        int target;
        if constexpr (EXCL) target = search.target[pr < n_pairs ? pr : 0];
        else if constexpr (SEARCH) target = *search.target;
        else target = deep.target;
        const bool open = (threadIdx.x & 63) < 32 * PB && pr < n_pairs && deep.state[pr].count < target;
        if (__ballot(open) == 0) return;
    }
    const int dp = 16 * ksteps;
    const int row_bytes = 4 * dp + 16;                                      // (the padding spreads the pairs' equal chunks over the banks)
    float* pinv = reinterpret_cast<float*>(smem + static_cast<size_t>(32 * PB) * row_bytes);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t pair0 = static_cast<int64_t>(blockIdx.x) * (32 * PB);
    // mixed rows m = lam F[q] + (1 - lam) F[u] (PredictionLayers.py:35) of this block's pairs, one wave per row: largest magnitude, scale, two fp16 planes;
    // pairs past the end repeat the last one
    for (int r = wave; r < 32 * PB; r += kEvalThreads / kWave) {
        int64_t pr = pair0 + r;
        pr = pr < n_pairs ? pr : n_pairs - 1;
        const float* qrow;
        const float* urow;
        [[maybe_unused]] int qd = dim;                                      // the columns the query row has in memory
        [[maybe_unused]] bool anon = false;                                 // (wave-uniform: one wave per row)
        if constexpr (SEARCH) {
            if (search.query_rows != nullptr) {
                qrow = search.query_rows + pr * search.ld_q;
                qd = search.q_dim;
            } else {
                qrow = feat + (queries[pr] + query_row0) * ld;
            }
            anon = users[pr] < 0;
            urow = feat + (anon ? 0 : users[pr]) * ld;                      // (never read for an anonymous pair; row 0 is there whatever happens)
        } else {
            qrow = feat + (queries[pr] + query_row0) * ld;
            urow = feat + users[pr] * ld;
        }
        const auto mixed = [&](int c) -> float {
            if constexpr (SEARCH) {
                const float q = c < qd ? qrow[c] : 0.f;
                if (anon) return q;
                return lam * q + (1.f - lam) * urow[c];
            } else {
                return lam * qrow[c] + (1.f - lam) * urow[c];
            }
        };
        float m = 0.f;
        [[maybe_unused]] float ss = 0.f;
        for (int c = lane; c < dim; c += kWave) {
            const float v = mixed(c);
            m = fmaxf(m, fabsf(v));
            if constexpr (COSINE) ss += v * v;
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) m = fmaxf(m, __shfl_xor(m, off));
        float inv;
        const float sc = eval_scale_up_for(m, inv);
        if constexpr (COSINE) {                                             // pinv = inverse scale / max(||m||, eps): the cosine's other factor
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) ss += __shfl_xor(ss, off);
            inv /= fmaxf(sqrtf(ss), kCosineEps);
        }
        if (lane == 0) pinv[r] = inv;
        for (int chunk = lane; chunk < 2 * ksteps; chunk += kWave) {
            float x[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int c = 8 * chunk + i;
                x[i] = c < dim ? mixed(c) * sc : 0.f;
            }
            v4u hi, lo;
            eval_split8(x, hi, lo);
            *reinterpret_cast<v4u*>(smem + static_cast<size_t>(r) * row_bytes + 16 * chunk) = hi;
            *reinterpret_cast<v4u*>(smem + static_cast<size_t>(r) * row_bytes + 2 * dp + 16 * chunk) = lo;
        }
    }
    __syncthreads();

    // this wave's run of 32-item tiles inside this block's item slice
    constexpr int WAVES = kEvalThreads / kWave;
    const int64_t n_tiles = (n_items + 31) / 32;
    const int64_t n_runs = static_cast<int64_t>(gridDim.y) * WAVES;
    const int64_t run = static_cast<int64_t>(blockIdx.y) * WAVES + wave;
    const int64_t tile_begin = n_tiles * run / n_runs, tile_end = n_tiles * (run + 1) / n_runs;
    const int n31 = lane & 31, half = lane >> 5;
    float my_pinv[PB];
    const unsigned char* brow[PB];
#pragma unroll
    for (int pb = 0; pb < PB; ++pb) {
        my_pinv[pb] = pinv[32 * pb + n31];
        brow[pb] = smem + static_cast<size_t>(32 * pb + n31) * row_bytes + 16 * half;
    }
    TopList top[PB];
#pragma unroll
    for (int pb = 0; pb < PB; ++pb) top[pb].init();
    [[maybe_unused]] float b_val[PB];
    [[maybe_unused]] int b_idx[PB];
    if constexpr (DEEP) {
#pragma unroll
        for (int pb = 0; pb < PB; ++pb) {
            int64_t pr = pair0 + 32 * pb + n31;
            pr = pr < n_pairs ? pr : n_pairs - 1;
            b_val[pb] = deep.state[pr].b_val;
            b_idx[pb] = deep.state[pr].b_idx;
        }
    }
    // EXCL: the cursor starts at the run's first id at or past this wave's first item (a lower bound, once per wave run); pairs past the end, which repeat the
    // last pair and write nothing, follow no run
    [[maybe_unused]] ExclCursor cur[PB];
    if constexpr (EXCL) {
#pragma unroll
        for (int pb = 0; pb < PB; ++pb) {
            const int64_t pr = pair0 + 32 * pb + n31;
            int64_t lo = 0, hi = 0;
            if (pr < n_pairs && tile_begin < tile_end) {
                const int64_t row = excl.row != nullptr ? excl.row[pr] : pr;
                if (row >= 0) {
                    lo = excl.ptr[row];
                    hi = excl.ptr[row + 1];
                }
            }
            cur[pb].end = excl.items + hi;
            const int64_t first = tile_begin * 32;
            while (lo < hi) {
                const int64_t mid = lo + (hi - lo) / 2;
                if (excl.items[mid] < first) lo = mid + 1; else hi = mid;
            }
            cur[pb].at = excl.items + lo;
            cur[pb].next = cur[pb].at < cur[pb].end ? *cur[pb].at : INT_MAX;
        }
    }

    constexpr int PF = 4;                                                   // k-steps of item fragments in flight
    for (int64_t tile = tile_begin; tile < tile_end; ++tile) {
        const v4u* af = frag + (tile * ksteps * 2) * kWave + lane;
        v16f acc[PB];
#pragma unroll
        for (int pb = 0; pb < PB; ++pb)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[pb][r] = 0.f;
        v4u a[PF][2];
#pragma unroll
        for (int x = 0; x < PF; ++x) {
            const int ks = x < ksteps ? x : ksteps - 1;
            a[x][0] = af[(2 * ks) * kWave];
            a[x][1] = af[(2 * ks + 1) * kWave];
        }
        for (int k0 = 0; k0 < ksteps; k0 += PF) {
#pragma unroll
            for (int x = 0; x < PF; ++x) {
                const int ks = k0 + x;
                if (ks < ksteps) {
                    const v8h ahi = __builtin_bit_cast(v8h, a[x][0]), alo = __builtin_bit_cast(v8h, a[x][1]);
                    const int nk = ks + PF < ksteps ? ks + PF : ksteps - 1;     // (past the end: the last k-step again, read and dropped)
                    a[x][0] = af[(2 * nk) * kWave];
                    a[x][1] = af[(2 * nk + 1) * kWave];
#pragma unroll
                    for (int pb = 0; pb < PB; ++pb) {
                        const v8h bhi = *reinterpret_cast<const v8h*>(brow[pb] + 32 * ks), blo = *reinterpret_cast<const v8h*>(brow[pb] + 2 * dp + 32 * ks);
                        acc[pb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ahi, blo, acc[pb], 0, 0, 0);
                        acc[pb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(alo, bhi, acc[pb], 0, 0, 0);
                        acc[pb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ahi, bhi, acc[pb], 0, 0, 0);
                    }
                }
            }
        }
        // this lane: pairs 32 pb + n31, items tile * 32 + acc_row(r, lane)
#pragma unroll
        for (int r4 = 0; r4 < 4; ++r4) {
            const int64_t i0 = tile * 32 + 8 * r4 + 4 * half;
            float2 ax[4];
#pragma unroll
            for (int x = 0; x < 4; ++x) ax[x] = i0 + x < n_items ? aux[i0 + x] : make_float2(0.f, 0.f);
            // EXCL: bit x of skip[pb] = item i0 + x is in the pair's run.  The ids of the other lane half (and of other waves' tiles) are stepped over; a lane
            // whose run has nothing before i0 + 4 - every lane of a call without lists - pays the one comparison
            [[maybe_unused]] unsigned skip[PB];
            if constexpr (EXCL) {
#pragma unroll
                for (int pb = 0; pb < PB; ++pb) {
                    skip[pb] = 0u;
                    if (cur[pb].next < i0 + 4) {
                        while (cur[pb].next < i0) cur[pb].step();
                        while (cur[pb].next < i0 + 4) {
                            skip[pb] |= 1u << (cur[pb].next - static_cast<int>(i0));
                            cur[pb].step();
                        }
                    }
                }
            }
#pragma unroll
            for (int x = 0; x < 4; ++x) {
                const int i = static_cast<int>(i0 + x);
#pragma unroll
                for (int pb = 0; pb < PB; ++pb) {
                    const float s = acc[pb][4 * r4 + x] * (ax[x].x * my_pinv[pb]) + ax[x].y;
                    if constexpr (EXCL) {
                        if (i0 + x < n_items && ((skip[pb] >> x) & 1u) == 0 && ranks_before(b_val[pb], b_idx[pb], s, i) &&
                            ranks_before(s, i, top[pb].val[kTopMax - 1], top[pb].idx[kTopMax - 1]))
                            top[pb].insert(s, i);
                    } else if constexpr (DEEP) {
                        if (i0 + x < n_items && ranks_before(b_val[pb], b_idx[pb], s, i) && ranks_before(s, i, top[pb].val[kTopMax - 1], top[pb].idx[kTopMax - 1])) top[pb].insert(s, i);
                    } else {
                        if (i0 + x < n_items && ranks_before(s, i, top[pb].val[kTopMax - 1], top[pb].idx[kTopMax - 1])) top[pb].insert(s, i);
                    }
                }
            }
        }
    }
    const int64_t n_lists = n_runs * 2;
#pragma unroll
    for (int pb = 0; pb < PB; ++pb) {
        const int64_t pair = pair0 + 32 * pb + n31;
        if (pair < n_pairs) {
            const int64_t base = (pair * n_lists + run * 2 + half) * kTopMax;
#pragma unroll
            for (int p = 0; p < kTopMax; ++p) {
                part_val[base + p] = top[pb].val[p];
                part_idx[base + p] = top[pb].idx[p];
            }
        }
    }
}

// one wave per pair: the best k of its n_lists * kTopMax candidates, best first
__global__ __launch_bounds__(kBlockThreads) void merge_topk_kernel(const float* __restrict__ part_val, const int32_t* __restrict__ part_idx,
                                                                   int64_t n_pairs, int n_cand, int k, float* __restrict__ out_val,
                                                                   int32_t* __restrict__ out_idx) {
    const int lane = threadIdx.x & 63;
    for (int64_t pair = global_wave_id(); pair < n_pairs; pair += global_wave_count()) {
    const float* pv = part_val + pair * n_cand;
    const int32_t* pi = part_idx + pair * n_cand;
    float last_v = FLT_MAX;
    int last_i = -1;
    for (int round = 0; round < k; ++round) {
        // best candidate that ranks strictly after the previous winner (candidates are distinct items, so "after" = not yet taken)
        float bv = -FLT_MAX;
        int bi = INT_MAX;
        for (int c = lane; c < n_cand; c += kWave) {
            const float v = pv[c];
            const int i = pi[c];
            if (ranks_before(last_v, last_i, v, i) && ranks_before(v, i, bv, bi)) {
                bv = v;
                bi = i;
            }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const float ov = __shfl_xor(bv, off);
            const int oi = __shfl_xor(bi, off);
            if (ranks_before(ov, oi, bv, bi)) {
                bv = ov;
                bi = oi;
            }
        }
        if (lane == 0) {
            out_val[pair * k + round] = bv;
            out_idx[pair * k + round] = bi == INT_MAX ? -1 : bi;
        }
        last_v = bv;
        last_i = bi;
    }
    }
}

// ------------------------------------------------------------------------------------------------
// Deep top-k (kTopMax < k <= kDeepMax) in passes; the lanes keep their lists of ten.  A pass = score_topk_kernel<PB, COSINE, true> (the candidates that rank after the
// pair's boundary) + merge_deep_kernel: the pair's n_lists lists are sorted best first over disjoint items, so with t = the best-ranking LAST entry over the full lists
// (a list with an empty slot hides nothing) every item that ranks at or before t is in some list, and the union of the lists is exact down to t.  The merge appends
// those candidates in order, stops at k, and moves the boundary to the last one appended.  A full list alone brings ten, so an incomplete pair gains at least ten ranks
// per pass: ceil(min(k, n_items) / 10) passes always suffice, and the host launches exactly that many - no read-back, no atomics, no spinning.
// ------------------------------------------------------------------------------------------------
constexpr int kDeepMax = 128;
constexpr int kDeepListsPerLane = 16;       // 64 slices x 8 waves x 2 lane halves = 1,024 lists at most (eval_slices)

// once per call: no rank emitted, every item after the boundary; the output holds the fill of merge_topk_kernel (-FLT_MAX, -1) wherever no rank will be written
__global__ __launch_bounds__(kBlockThreads) void deep_init_kernel(DeepState* __restrict__ state, int64_t n_pairs, int k, float* __restrict__ out_val, int32_t* __restrict__ out_idx) {
    const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
    for (int64_t t = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; t < n_pairs * k; t += stride) {
        out_val[t] = -FLT_MAX;
        out_idx[t] = -1;
        if (t < n_pairs) state[t] = DeepState{__builtin_inff(), -1, 0, 0};
    }
}

// one wave per incomplete pair.  Lane l owns lists l, l + 64, ...: the head of each in registers (statically indexed: no scratch), the best head of the wave by
// shuffles, and the one lane that owned it loads its list's next entry - one load per emitted rank, where k full scans of the candidates would be k x n_lists x 10.
// SEARCH: `target` is read from search.target (min(k, candidates), formed on the device); EXCL: from search.target[pair].  An excluded item is in no list, so the
// lists are exact over the pair's remaining candidates down to t and the argument above holds for them: a pair short of target[pair] still gains ten ranks or all
// that is left, and the ceil(min(k, n_items) / 10) passes the host launches are at least ceil(target[pair] / 10).  Past the last rank the row keeps deep_init's tail.
template <bool SEARCH = false, bool EXCL = false>
__global__ __launch_bounds__(kBlockThreads) void merge_deep_kernel(const float* __restrict__ part_val, const int32_t* __restrict__ part_idx, int64_t n_pairs, int n_lists, int k,
                                                                    int target, DeepState* __restrict__ state, float* __restrict__ out_val, int32_t* __restrict__ out_idx,
                                                                    int32_t* __restrict__ passes, [[maybe_unused]] const SearchArgs<SEARCH> search) {
    static_assert(SEARCH || !EXCL, "the per-pair target rides on the search arguments");
    const int lane = threadIdx.x & 63;
    if constexpr (SEARCH && !EXCL) target = *search.target;
    for (int64_t pair = global_wave_id(); pair < n_pairs; pair += global_wave_count()) {
        if constexpr (EXCL) target = search.target[pair];
        const DeepState st = state[pair];
        if (st.count >= target) continue;                                   // complete (wave-uniform): its lists are stale and its output is final
        const float* pv = part_val + pair * n_lists * kTopMax;
        const int32_t* pi = part_idx + pair * n_lists * kTopMax;
        float hv[kDeepListsPerLane];
        int hi[kDeepListsPerLane], pos[kDeepListsPerLane];
        float tv = -FLT_MAX;                                                // t: nothing ranks after (-FLT_MAX, INT_MAX), so with no full list every candidate is taken
        int ti = INT_MAX;
#pragma unroll
        for (int j = 0; j < kDeepListsPerLane; ++j) {
            const int list = lane + kWave * j;
            hv[j] = -FLT_MAX;
            hi[j] = INT_MAX;
            pos[j] = 0;
            if (list < n_lists) {
                hv[j] = pv[list * kTopMax];
                hi[j] = pi[list * kTopMax];
                const float lv = pv[list * kTopMax + kTopMax - 1];
                const int li = pi[list * kTopMax + kTopMax - 1];
                if (li != INT_MAX && ranks_before(lv, li, tv, ti)) {
                    tv = lv;
                    ti = li;
                }
            }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const float ov = __shfl_xor(tv, off);
            const int oi = __shfl_xor(ti, off);
            if (ranks_before(ov, oi, tv, ti)) {
                tv = ov;
                ti = oi;
            }
        }
#pragma unroll
        for (int j = 0; j < kDeepListsPerLane; ++j)
            if (ranks_before(tv, ti, hv[j], hi[j])) hi[j] = INT_MAX;        // a head after t: the list has nothing more to give (an empty head has INT_MAX already)
        int count = st.count;
        float last_v = st.b_val;
        int last_i = st.b_idx;
        while (count < k) {
            float bv = -FLT_MAX;
            int bi = INT_MAX, bj = 0;
#pragma unroll
            for (int j = 0; j < kDeepListsPerLane; ++j)
                if (hi[j] != INT_MAX && (bi == INT_MAX || ranks_before(hv[j], hi[j], bv, bi))) {
                    bv = hv[j];
                    bi = hi[j];
                    bj = j;
                }
            float wv = bv;
            int wi = bi;
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                const float ov = __shfl_xor(wv, off);
                const int oi = __shfl_xor(wi, off);
                if (oi != INT_MAX && (wi == INT_MAX || ranks_before(ov, oi, wv, wi))) {
                    wv = ov;
                    wi = oi;
                }
            }
            if (wi == INT_MAX) break;                                       // every list is spent down to t
            if (lane == 0) {
                out_val[pair * k + count] = wv;
                out_idx[pair * k + count] = wi;
            }
            ++count;
            last_v = wv;
            last_i = wi;
            if (bi == wi) {                                                 // the one lane that held the winner (items are distinct across lists): its list's next entry
#pragma unroll
                for (int j = 0; j < kDeepListsPerLane; ++j)
                    if (j == bj) {
                        const int np = pos[j] + 1;
                        float nv = -FLT_MAX;
                        int ni = INT_MAX;
                        if (np < kTopMax) {
                            const int at = (lane + kWave * j) * kTopMax + np;
                            nv = pv[at];
                            ni = pi[at];
                            if (ranks_before(tv, ti, nv, ni)) ni = INT_MAX;
                        }
                        pos[j] = np;
                        hv[j] = nv;
                        hi[j] = ni;
                    }
            }
        }
        if (lane == 0) {
            state[pair] = DeepState{last_v, last_i, count, st.passes + 1};
            if (passes != nullptr) passes[pair] = st.passes + 1;                // (every pair is incomplete in the first pass: each passes[c] is written)
        }
    }
}

// once per ihg_search_topk call, one workgroup: *target = min(k, the candidates among the first n_items bits of the mask) - the deep kernels read it where the plain
// deep call passes min(k, n_items) by value - and passes[c] = 0 (with no candidate no pass finds a pair incomplete, and merge_deep_kernel writes nothing)
__global__ __launch_bounds__(kBlockThreads) void search_target_kernel(const uint32_t* __restrict__ item_mask, int64_t n_items, int k, int32_t* __restrict__ target,
                                                                      int32_t* __restrict__ passes, int64_t n_pairs) {
    __shared__ int part[kWavesPerBlock];
    const int tid = threadIdx.x;
    if (passes != nullptr)
        for (int64_t c = tid; c < n_pairs; c += kBlockThreads) passes[c] = 0;
    int64_t count = n_items;
    if (item_mask != nullptr) {
        const int64_t n_words = (n_items + 31) / 32;
        int mine = 0;                                                        // (at most k + 31 bits matter, but the words are few: 3,750 at 120,000 items)
        for (int64_t w = tid; w < n_words; w += kBlockThreads) {
            uint32_t bits = item_mask[w];
            if (w == n_words - 1 && (n_items & 31) != 0) bits &= (1u << (n_items & 31)) - 1u;      // bits at or past n_items are ignored
            mine += __popc(bits);
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) mine += __shfl_xor(mine, off);
        if ((tid & 63) == 0) part[tid >> 6] = mine;
        __syncthreads();
        count = 0;
        for (int w = 0; w < kWavesPerBlock; ++w) count += part[w];
    }
    if (tid == 0) *target = static_cast<int32_t>(count < k ? count : k);
}

// once per ihg_search_topk_excluding call, after search_target_kernel has left the candidates' count in *n_candidates (its k = INT_MAX), one wave per pair:
// target[c] = min(k, candidates - the ids of the pair's run that are candidates) - an excluded id that the mask already removes is not subtracted twice, and the
// run is strictly ascending, so no id is counted twice either.  An id outside [0, n_items) is the caller's breach of contract; it is skipped here, not read through.
__global__ __launch_bounds__(kBlockThreads) void exclude_target_kernel(const uint32_t* __restrict__ item_mask, int64_t n_items, int k, const int32_t* __restrict__ n_candidates,
                                                                       const ExclArgs<true> excl, int32_t* __restrict__ target, int64_t n_pairs) {
    const int lane = threadIdx.x & 63;
    const int candidates = *n_candidates;
    for (int64_t pair = global_wave_id(); pair < n_pairs; pair += global_wave_count()) {
        const int64_t row = excl.row != nullptr ? excl.row[pair] : pair;    // (wave-uniform)
        int hits = 0;
        if (row >= 0) {
            const int64_t end = excl.ptr[row + 1];
            for (int64_t e = excl.ptr[row] + lane; e < end; e += kWave) {
                const int64_t i = excl.items[e];
                if (i >= 0 && i < n_items && (item_mask == nullptr || ((item_mask[i >> 5] >> (i & 31)) & 1u) != 0)) ++hits;
            }
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) hits += __shfl_xor(hits, off);
        const int left = candidates - hits;
        if (lane == 0) target[pair] = left < k ? left : k;
    }
}

// ------------------------------------------------------------------------------------------------
// Host side.  Every entry point below fills a RankCall (ranking.hpp) and hands it to catalogue_rank with its rules and its shape: the shared front in the shared
// order, the workspace from the one layout function (eval_workspace), and the launch routine of the call's (shape, head) out of one table.
// ------------------------------------------------------------------------------------------------
constexpr int kEvalWavesPerBlock = kEvalThreads / kWave;
constexpr size_t kEvalLds = 160 * 1024;

constexpr int eval_ksteps(int dim) { return (dim + 15) / 16; }
constexpr size_t eval_lds_bytes(int dim, int pb) { return static_cast<size_t>(32 * pb) * (4 * 16 * eval_ksteps(dim) + 16) + static_cast<size_t>(32 * pb) * sizeof(float); }
inline int eval_pair_tiles(int dim) { return eval_lds_bytes(dim, 2) <= kEvalLds ? 2 : 1; }      // pair tiles of 32 per workgroup
// the widest feature row whose 32-pair block (two fp16 planes + the row pad + the pair scales) fits the 160 KB of LDS: 1264 (79 k-steps of 16)
constexpr int eval_max_dim() {
    int dim = 16;
    while (eval_lds_bytes(dim + 16, 1) <= kEvalLds) dim += 16;
    return dim;
}

inline int eval_slices(int64_t n_pairs, int64_t n_items, int dim) {
    const int64_t blocks = (n_pairs + 32 * eval_pair_tiles(dim) - 1) / (32 * eval_pair_tiles(dim));
    const int64_t tiles = (n_items + 31) / 32;
    int64_t slices = (512 + blocks - 1) / blocks;                           // ~2 workgroups per CU in all (one resident per CU: LDS)
    const int64_t most = std::max<int64_t>(1, tiles / (kEvalWavesPerBlock * 4));    // at least 4 tiles per wave
    slices = std::max<int64_t>(1, std::min<int64_t>({slices, most, 64}));
    return static_cast<int>(slices);
}
inline int64_t eval_lists(int64_t n_pairs, int64_t n_items, int dim) { return static_cast<int64_t>(eval_slices(n_pairs, n_items, dim)) * kEvalWavesPerBlock * 2; }

// The workspace of every catalogue entry point, region after region: the item fragments | aux | the partial lists' values | their ids | deep: DeepState per pair |
// search: the 16-byte cell of search_target_kernel | excluding: target[n_pairs] of exclude_target_kernel, rounded up to 16 bytes.  A search without lists reads its
// ranks from the cell itself.  A null base answers the size query (`bytes`), the caller's pointer carves the regions: the two cannot drift.
struct EvalWorkspace {
    v4u* frag;
    float2* aux;
    float* part_val;
    int32_t* part_idx;
    DeepState* state;
    int32_t *target_cell, *target;
    int64_t bytes;
};
inline EvalWorkspace eval_workspace(void* base, int64_t n_pairs, int64_t n_items, int dim, bool deep, bool search, bool excluding) {
    const int64_t tiles = (n_items + 31) / 32, entries = n_pairs * eval_lists(n_pairs, n_items, dim) * kTopMax;
    WorkspaceCursor ws(base);
    EvalWorkspace w{};
    w.frag = static_cast<v4u*>(ws.take(tiles * eval_ksteps(dim) * 2 * kWave * 16));
    w.aux = static_cast<float2*>(ws.take(tiles * 32 * 8));
    w.part_val = static_cast<float*>(ws.take(entries * 4));
    w.part_idx = static_cast<int32_t*>(ws.take(entries * 4));
    if (deep) w.state = static_cast<DeepState*>(ws.take(n_pairs * static_cast<int64_t>(sizeof(DeepState))));
    if (search) w.target = w.target_cell = static_cast<int32_t*>(ws.take(16));
    if (excluding) w.target = static_cast<int32_t*>(ws.take(align16(n_pairs * 4)));
    w.bytes = ws.at;
    return w;
}

// The scoring kernel of a call: PB = 2 pair tiles per workgroup where their planes fit LDS, and the opt-in to more than 64 KB of it - once per device ordinal (it
// belongs to the device's code object) and per instantiation: the flags are a static of this template, which is instantiated once per kernel pair.
template <bool COSINE, bool DEEP, bool SEARCH, bool EXCL>
auto score_topk_kernel_for(int pb) {
    const auto one = score_topk_kernel<1, COSINE, DEEP, SEARCH, EXCL>, two = score_topk_kernel<2, COSINE, DEEP, SEARCH, EXCL>;
    static bool attr_set[64] = {};
    int device = 0;
    if (hipGetDevice(&device) != hipSuccess) (void)hipGetLastError();
    if (device < 0 || device >= 64 || !attr_set[device]) {
        for (const void* kernel : {reinterpret_cast<const void*>(one), reinterpret_cast<const void*>(two)})
            if (hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, kEvalLds) != hipSuccess) (void)hipGetLastError();
        if (device >= 0 && device < 64) attr_set[device] = true;
    }
    return pb == 2 ? two : one;
}

// The launches of one call.  Plain (DEEP = false): prepare -> score -> merge_topk_kernel.  Deep: the targets (SEARCH: on the device) -> prepare -> deep_init ->
// ceil(min(k, n_items) / 10) passes of (score, merge_deep_kernel).
template <bool COSINE, bool DEEP, bool SEARCH, bool EXCL>
int catalogue_launch(const char* what, const RankCall& c) {
    hipStream_t s = static_cast<hipStream_t>(c.stream);
    const int ksteps = eval_ksteps(c.dim), pb = eval_pair_tiles(c.dim);
    const int slices = eval_slices(c.n_pairs, c.n_items, c.dim);
    const int n_lists = static_cast<int>(eval_lists(c.n_pairs, c.n_items, c.dim));
    const EvalWorkspace ws = eval_workspace(c.workspace, c.n_pairs, c.n_items, c.dim, DEEP, SEARCH, EXCL);
    const int target = static_cast<int>(std::min<int64_t>(c.k, c.n_items));        // (SEARCH: the most a mask leaves - the passes launched; the kernels read search.target)
    SearchArgs<SEARCH> search{};
    ExclArgs<EXCL> excl{};
    DeepArgs<DEEP> deep{};
    if constexpr (SEARCH) {
        search = SearchArgs<true>{c.query_rows, c.ld_q, c.q_dim, c.item_mask, ws.target};
        // EXCL: the cell holds the candidates' count itself, and exclude_target_kernel forms target[n_pairs] from it
        hipLaunchKernelGGL(search_target_kernel, dim3(1), dim3(kBlockThreads), 0, s, c.item_mask, c.n_items, EXCL ? INT_MAX : c.k, ws.target_cell, c.passes, c.n_pairs);
        if constexpr (EXCL) {
            excl = ExclArgs<true>{c.excl_ptr, c.excl_items, c.excl_row};
            hipLaunchKernelGGL(exclude_target_kernel, dim3(grid_for_waves(c.n_pairs)), dim3(kBlockThreads), 0, s, c.item_mask, c.n_items, c.k, ws.target_cell, excl, ws.target, c.n_pairs);
        }
    }
    hipLaunchKernelGGL((score_prepare_kernel<COSINE, SEARCH>), dim3(grid_for_waves(c.n_items)), dim3(kBlockThreads), 0, s, c.features, c.ld, c.dim, ksteps, c.item_row0, c.n_items, c.item_bias,
                       ws.frag, ws.aux, search);
    if constexpr (DEEP) {
        deep = DeepArgs<true>{ws.state, target};
        hipLaunchKernelGGL(deep_init_kernel, dim3(static_cast<unsigned>(std::min<int64_t>((c.n_pairs * c.k + kBlockThreads - 1) / kBlockThreads, 4096))), dim3(kBlockThreads), 0, s, ws.state,
                           c.n_pairs, c.k, c.top_scores, c.top_items);
    }
    const auto score = score_topk_kernel_for<COSINE, DEEP, SEARCH, EXCL>(pb);
    const dim3 grid(static_cast<unsigned>((c.n_pairs + 32 * pb - 1) / (32 * pb)), slices);
    const int n_passes = DEEP ? (target + kTopMax - 1) / kTopMax : 1;
    for (int pass = 0; pass < n_passes; ++pass) {
        hipLaunchKernelGGL(score, grid, dim3(kEvalThreads), eval_lds_bytes(c.dim, pb), s, c.features, c.ld, c.dim, ksteps, ws.frag, ws.aux, c.n_items, c.users, c.queries, c.query_row0,
                           c.lambda_muq, c.n_pairs, ws.part_val, ws.part_idx, deep, search, excl);
        if constexpr (DEEP)
            hipLaunchKernelGGL((merge_deep_kernel<SEARCH, EXCL>), dim3(grid_for_waves(c.n_pairs)), dim3(kBlockThreads), 0, s, ws.part_val, ws.part_idx, c.n_pairs, n_lists, c.k, target, ws.state,
                               c.top_scores, c.top_items, c.passes, search);
        else
            hipLaunchKernelGGL(merge_topk_kernel, dim3(grid_for_waves(c.n_pairs)), dim3(kBlockThreads), 0, s, ws.part_val, ws.part_idx, c.n_pairs, n_lists * kTopMax, c.k, c.top_scores,
                               c.top_items);
    }
    return check_launch(what);
}

// An entry point is its rules for the front and the first of its launch shapes, which also says what regions its workspace has (kExcluding: target[n_pairs]; a call of
// that entry without lists launches kSearch).
enum CatalogueShape { kPlain, kDeep, kSearch, kExcluding };
constexpr const char* kPairBlock = "does not fit the LDS pair block";
constexpr RankRules kScoreTopk{"ihg_score_topk", kTopMax, "", false, eval_max_dim(), kPairBlock, IHG_ERR_WORKSPACE};
constexpr RankRules kScoreTopkCosine{"ihg_score_topk_cosine", kTopMax, "", false, eval_max_dim(), kPairBlock, IHG_ERR_WORKSPACE};
constexpr RankRules kScoreTopkDeep{"ihg_score_topk_deep", kDeepMax, "1 <= ", false, eval_max_dim(), kPairBlock, IHG_ERR_WORKSPACE};
constexpr RankRules kSearchTopk{"ihg_search_topk", kDeepMax, "1 <= ", true, eval_max_dim(), kPairBlock, IHG_ERR_INVALID};
constexpr RankRules kSearchTopkExcluding{"ihg_search_topk_excluding", kDeepMax, "1 <= ", true, eval_max_dim(), kPairBlock, IHG_ERR_INVALID};

inline int64_t catalogue_workspace_bytes(CatalogueShape shape, int64_t n_pairs, int64_t n_items, int dim, int k) {
    if (n_pairs <= 0 || n_items <= 0 || dim <= 0 || (shape != kPlain && (k <= 0 || k > kDeepMax))) return 0;
    return eval_workspace(nullptr, n_pairs, n_items, dim, shape >= kDeep, shape >= kSearch, shape >= kExcluding).bytes;
}

// the run-time (shape, head) -> the template instance: the one dispatch
using CatalogueLaunch = int (*)(const char*, const RankCall&);
constexpr CatalogueLaunch kCatalogueLaunch[4][2] = {{catalogue_launch<false, false, false, false>, catalogue_launch<true, false, false, false>},
                                                    {catalogue_launch<false, true, false, false>, catalogue_launch<true, true, false, false>},
                                                    {catalogue_launch<false, true, true, false>, catalogue_launch<true, true, true, false>},
                                                    {catalogue_launch<false, true, true, true>, catalogue_launch<true, true, true, true>}};

int catalogue_rank(const RankCall& c, const RankRules& r, CatalogueShape shape) {
    if (int rc = rank_check_call(c, r)) return rc;
    if (c.n_pairs == 0) return IHG_OK;
    if (int rc = rank_check_pointers(c, r)) return rc;
    if (shape != kPlain && eval_lists(c.n_pairs, c.n_items, c.dim) > kWave * kDeepListsPerLane) return fail(IHG_ERR_INVALID, "%s: more partial lists than the merge holds", r.what);
    if (int rc = rank_check_workspace(c, r, catalogue_workspace_bytes(shape, c.n_pairs, c.n_items, c.dim, c.k))) return rc;
    if (shape == kExcluding && c.excl_ptr == nullptr) shape = kSearch;      // no lists: the launches of ihg_search_topk
    return kCatalogueLaunch[shape][c.cosine != 0](r.what, c);
}

}  // namespace

extern "C" {

int32_t ihg_score_topk_max_dim(void) { return eval_max_dim(); }
int32_t ihg_score_topk_max_k(void) { return kDeepMax; }

// regions: fragments | aux | partial values | partial ids
int64_t ihg_score_topk_workspace_bytes(int64_t n_pairs, int64_t n_items, int32_t dim) { return catalogue_workspace_bytes(kPlain, n_pairs, n_items, dim, 0); }
// ... | DeepState[n_pairs]
int64_t ihg_score_topk_deep_workspace_bytes(int64_t n_pairs, int64_t n_items, int32_t dim, int32_t k) { return catalogue_workspace_bytes(kDeep, n_pairs, n_items, dim, k); }
// ... | the target cell (16 bytes)
int64_t ihg_search_topk_workspace_bytes(int64_t n_pairs, int64_t n_items, int32_t dim, int32_t k) { return catalogue_workspace_bytes(kSearch, n_pairs, n_items, dim, k); }
// ... | target[n_pairs] (rounded up to 16 bytes)
int64_t ihg_search_topk_excluding_workspace_bytes(int64_t n_pairs, int64_t n_items, int32_t dim, int32_t k) { return catalogue_workspace_bytes(kExcluding, n_pairs, n_items, dim, k); }

int ihg_score_topk(const float* features, int64_t ld, int32_t dim, int64_t query_row0, int64_t item_row0, int64_t n_items, const float* item_bias,
                   const int64_t* users, const int64_t* queries, float lambda_muq, int64_t n_pairs, int32_t k, float* top_scores,
                   int32_t* top_items, void* workspace, int64_t workspace_bytes, ihg_stream_t stream) {
    RankCall c;
    c.features = features, c.ld = ld, c.dim = dim, c.query_row0 = query_row0, c.item_row0 = item_row0, c.n_items = n_items, c.item_bias = item_bias;
    c.users = users, c.queries = queries, c.lambda_muq = lambda_muq, c.n_pairs = n_pairs, c.k = k, c.top_scores = top_scores, c.top_items = top_items;
    c.workspace = workspace, c.workspace_bytes = workspace_bytes, c.stream = stream;
    return catalogue_rank(c, kScoreTopk, kPlain);
}

// the cosine head: the same kernels with the rows' inverse norms folded into the two scale factors (score_prepare_kernel<true>, score_topk_kernel<PB, true>)
int ihg_score_topk_cosine(const float* features, int64_t ld, int32_t dim, int64_t query_row0, int64_t item_row0, int64_t n_items, const float* item_bias,
                   const int64_t* users, const int64_t* queries, float lambda_muq, int64_t n_pairs, int32_t k, float* top_scores,
                   int32_t* top_items, void* workspace, int64_t workspace_bytes, ihg_stream_t stream) {
    RankCall c;
    c.features = features, c.ld = ld, c.dim = dim, c.query_row0 = query_row0, c.item_row0 = item_row0, c.n_items = n_items, c.item_bias = item_bias;
    c.users = users, c.queries = queries, c.lambda_muq = lambda_muq, c.n_pairs = n_pairs, c.k = k, c.top_scores = top_scores, c.top_items = top_items;
    c.workspace = workspace, c.workspace_bytes = workspace_bytes, c.cosine = 1, c.stream = stream;
    return catalogue_rank(c, kScoreTopkCosine, kPlain);
}

int ihg_score_topk_deep(const float* features, int64_t ld, int32_t dim, int64_t query_row0, int64_t item_row0, int64_t n_items, const float* item_bias,
                        const int64_t* users, const int64_t* queries, float lambda_muq, int64_t n_pairs, int32_t k, float* top_scores,
                        int32_t* top_items, void* workspace, int64_t workspace_bytes, int32_t cosine, int32_t* passes, ihg_stream_t stream) {
    RankCall c;
    c.features = features, c.ld = ld, c.dim = dim, c.query_row0 = query_row0, c.item_row0 = item_row0, c.n_items = n_items, c.item_bias = item_bias;
    c.users = users, c.queries = queries, c.lambda_muq = lambda_muq, c.n_pairs = n_pairs, c.k = k, c.top_scores = top_scores, c.top_items = top_items;
    c.workspace = workspace, c.workspace_bytes = workspace_bytes, c.cosine = cosine, c.passes = passes, c.stream = stream;
    return catalogue_rank(c, kScoreTopkDeep, kDeep);
}

int ihg_search_topk(const float* features, int64_t ld, int32_t dim, int64_t query_row0, int64_t item_row0, int64_t n_items, const float* item_bias,
                    const int64_t* users, const int64_t* queries, const float* query_rows, int64_t ld_q, int32_t q_dim, const uint32_t* item_mask,
                    float lambda_muq, int64_t n_pairs, int32_t k, float* top_scores, int32_t* top_items, void* workspace, int64_t workspace_bytes,
                    int32_t cosine, int32_t* passes, ihg_stream_t stream) {
    RankCall c;
    c.features = features, c.ld = ld, c.dim = dim, c.query_row0 = query_row0, c.item_row0 = item_row0, c.n_items = n_items, c.item_bias = item_bias;
    c.users = users, c.queries = queries, c.query_rows = query_rows, c.ld_q = ld_q, c.q_dim = q_dim, c.item_mask = item_mask;
    c.lambda_muq = lambda_muq, c.n_pairs = n_pairs, c.k = k, c.top_scores = top_scores, c.top_items = top_items;
    c.workspace = workspace, c.workspace_bytes = workspace_bytes, c.cosine = cosine, c.passes = passes, c.stream = stream;
    return catalogue_rank(c, kSearchTopk, kSearch);
}

int ihg_search_topk_excluding(const float* features, int64_t ld, int32_t dim, int64_t query_row0, int64_t item_row0, int64_t n_items, const float* item_bias,
                              const int64_t* users, const int64_t* queries, const float* query_rows, int64_t ld_q, int32_t q_dim, const uint32_t* item_mask,
                              const int64_t* excl_ptr, const int32_t* excl_items, const int64_t* excl_row, int64_t n_excl_rows, float lambda_muq, int64_t n_pairs,
                              int32_t k, float* top_scores, int32_t* top_items, void* workspace, int64_t workspace_bytes, int32_t cosine, int32_t* passes,
                              ihg_stream_t stream) {
    RankCall c;
    c.features = features, c.ld = ld, c.dim = dim, c.query_row0 = query_row0, c.item_row0 = item_row0, c.n_items = n_items, c.item_bias = item_bias;
    c.users = users, c.queries = queries, c.query_rows = query_rows, c.ld_q = ld_q, c.q_dim = q_dim, c.item_mask = item_mask;
    c.excl_ptr = excl_ptr, c.excl_items = excl_items, c.excl_row = excl_row, c.n_excl_rows = n_excl_rows;
    c.lambda_muq = lambda_muq, c.n_pairs = n_pairs, c.k = k, c.top_scores = top_scores, c.top_items = top_items;
    c.workspace = workspace, c.workspace_bytes = workspace_bytes, c.cosine = cosine, c.passes = passes, c.stream = stream;
    return catalogue_rank(c, kSearchTopkExcluding, kExcluding);
}

}  // extern "C"
