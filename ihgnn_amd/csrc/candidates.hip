// candidates.hip - re-ranking a shortlist per search (ihg_search_candidates): every search names its own run of item ids and only those are scored, so the work is
// sum_c |run_c| * dim with no pass over the catalogue - no prepare pass, no split planes, nothing proportional to n_items (eval.hip's entry points stream every item
// row past every pair block).
//
// Arithmetic: plain fp32.  The mixed row m = lam q + (1 - lam) u of a search (SearchArgs' rules of eval.hip: q alone without a user, zero past q_dim for an external
// row) is formed once per (search, chunk of its run) into LDS; a group of G lanes (G by the row's width, cand_group_width) owns a candidate, lane g of it takes the
// 16-byte segments g, g + G, ... of the item row in ONE fma chain, the G partial sums meet in a shuffle tree, and the score is dot + bias[item] - or, under the
// cosine head, dot / (max(||a||, 1e-8) max(||m||, 1e-8)) + bias[item] with both sums of squares taken in the same order (tail.hip hem_cosine_fwd_kernel's formula).
// The scores are therefore NOT the bits of ihg_search_topk (two fp16 terms per operand on the matrix cores); tests/candidates_reference.py has the bound.
//
// Launches (no atomics, no host read, every output slot written):
//   cand_plan_kernel    per search: its run (begin, length) and whether it is the run's OWNER - the lowest-numbered search that names it
//   cand_units_kernel   one workgroup: the exclusive scan of the owners' chunk counts - unit u of the scoring pass is (search, chunk of kCandChunk ids)
//   cand_score_kernel   a wave per unit: the chunk's scores at their CSR slots (all_scores, or the workspace); the mask and the exclusion run write -inf
//   cand_select_kernel  a wave per search: every lane keeps a TopList of ten over its strided share of the run (entries that rank strictly after the search's
//                       boundary), the wave emits the best ten of the 64 lists and moves the boundary: ceil(target / 10) trips.  A search that is not the owner of
//                       its run has no stored scores (a slot holds one search's): its wave scores the run itself, chunk by chunk into LDS, with the same function.
// Host side: the call record, the argument checks and the list type are eval.hip's (ranking.hpp); cand_workspace lays the workspace out, cand_args fills the kernels' block.
#include "ranking.hpp"

namespace {

constexpr int kCandMaxK = 128;
constexpr int kCandChunk = 256;             // ids per scoring unit
constexpr int kCandMaxDim = 2048;           // the widest mixed row the LDS image takes
constexpr int kCandRows = 4;                // item rows in flight per lane group
constexpr int kCandMaxGrid = 256 * 16;      // one-wave workgroups: 16 per CU, grid-stride beyond that

// the run of a search as the kernels read it
struct CandRun {
    int64_t begin;                          // first CSR slot
    int32_t len;                            // 0: no run (a row outside [0, n_cand_rows), or offsets that do not lie inside [0, total])
    int32_t owner;                          // 1: the scores of this search are stored at the run's slots
};

// everything about the sources that both kernels need (by value: one kernel-argument block)
struct CandArgs {
    const float* feat;
    int64_t ld;
    int dim;
    int group;                              // G: lanes per candidate, a power of two <= 16
    int vec;                                // 1: every row starts on 16 bytes (features aligned, ld % 4 == 0)
    int64_t query_row0, item_row0, n_items;
    const float* bias;
    const int64_t* users;
    const int64_t* queries;
    const float* query_rows;
    int64_t ld_q;
    int q_dim;
    const uint32_t* item_mask;
    const int64_t* excl_ptr;
    const int32_t* excl_items;
    const int64_t* excl_row;
    int64_t n_excl_rows;
    const int32_t* cand_items;
    float lam;
};

inline int cand_group_width(int dim) {      // lanes per candidate: one 16-byte segment each up to 64 columns (a 256-byte row), then 16 lanes walk the row
    const int segs = (dim + 3) / 4;
    int g = 1;
    while (g < segs && g < 16) g *= 2;
    return g;
}

// m into LDS (columns dim .. the next multiple of four are zero); returns max(||m||, eps) under the cosine head (the group's chain and tree: the order of the item rows' sums)
template <bool COSINE>
__device__ float cand_mixed_row(const CandArgs& a, int64_t c, float* __restrict__ mrow) {
    const int lane = threadIdx.x & 63;
    const float* qrow;
    int qd = a.dim;
    if (a.query_rows != nullptr) {
        qrow = a.query_rows + c * a.ld_q;
        qd = a.q_dim;
    } else {
        qrow = a.feat + (a.queries[c] + a.query_row0) * a.ld;
    }
    const int64_t user = a.users[c];
    const bool anon = user < 0;
    const float* urow = a.feat + (anon ? 0 : user) * a.ld;                  // (never read for an anonymous search)
    const int dimp = (a.dim + 3) & ~3;
    __syncthreads();                                                         // (one wave per workgroup: the previous readers of mrow are done)
    for (int col = lane; col < dimp; col += kWave) {
        float v = 0.f;
        if (col < a.dim) {
            const float q = col < qd ? qrow[col] : 0.f;
            v = anon ? q : fmaf(a.lam, q, (1.f - a.lam) * urow[col]);
        }
        mrow[col] = v;
    }
    __syncthreads();
    if constexpr (!COSINE) return 1.f;
    const int g = lane & (a.group - 1), segs = dimp >> 2;
    float ss = 0.f;
    for (int s = g; s < segs; s += a.group) {
        const float4 m = *reinterpret_cast<const float4*>(mrow + 4 * s);
        ss = fmaf(m.x, m.x, ss);
        ss = fmaf(m.y, m.y, ss);
        ss = fmaf(m.z, m.z, ss);
        ss = fmaf(m.w, m.w, ss);
    }
    for (int off = a.group >> 1; off >= 1; off >>= 1) ss += __shfl_xor(ss, off);
    return fmaxf(sqrtf(ss), kCosineEps);
}

__device__ __forceinline__ float4 cand_segment(const float* __restrict__ row, int s, int dim, bool vec) {
    const int col = 4 * s;
    if (vec && col + 4 <= dim) return *reinterpret_cast<const float4*>(row + col);
    float4 x;
    x.x = col < dim ? row[col] : 0.f;
    x.y = col + 1 < dim ? row[col + 1] : 0.f;
    x.z = col + 2 < dim ? row[col + 2] : 0.f;
    x.w = col + 3 < dim ? row[col + 3] : 0.f;
    return x;
}

// the exclusion run of search c: [lo, hi) into excl_items (empty: none)
__device__ __forceinline__ void cand_excl_run(const CandArgs& a, int64_t c, int64_t& lo, int64_t& hi) {
    lo = hi = 0;
    if (a.excl_ptr == nullptr) return;
    const int64_t row = a.excl_row != nullptr ? a.excl_row[c] : c;
    if (row < 0 || row >= a.n_excl_rows) return;
    lo = a.excl_ptr[row];
    hi = a.excl_ptr[row + 1];
}

// Scores of `n` <= kCandChunk entries of a run (`ids`) for the search whose mixed row is in `mrow`, to out[0 .. n): the whole wave, (64 / G) x kCandRows candidates per
// step.  An id outside [0, n_items), outside the mask or in [xlo, xhi) of the exclusion list gets -inf and its row is not read.
template <bool COSINE>
__device__ void cand_score_chunk(const CandArgs& a, const float* __restrict__ mrow, float norm_m, const int32_t* __restrict__ ids, int n, int64_t xlo, int64_t xhi,
                                 float* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int G = a.group, g = lane & (G - 1), grp = lane / G, groups = kWave / G;
    const int segs = (a.dim + 3) >> 2;
    const bool vec = a.vec != 0;
    for (int base = 0; base < n; base += groups * kCandRows) {
        const float* row[kCandRows];
        int item[kCandRows];
        bool live[kCandRows];
#pragma unroll
        for (int r = 0; r < kCandRows; ++r) {
            const int e = base + r * groups + grp;
            item[r] = e < n ? ids[e] : -1;
            live[r] = item[r] >= 0 && item[r] < a.n_items;
            if (live[r] && a.item_mask != nullptr) live[r] = ((a.item_mask[item[r] >> 5] >> (item[r] & 31)) & 1u) != 0;
            if (live[r] && xlo < xhi) {                                      // the first excluded id at or past the item (both runs ascend; the run is short: a search)
                int64_t lo = xlo, hi = xhi;
                while (lo < hi) {
                    const int64_t mid = lo + (hi - lo) / 2;
                    if (a.excl_items[mid] < item[r]) lo = mid + 1; else hi = mid;
                }
                live[r] = !(lo < xhi && a.excl_items[lo] == item[r]);
            }
            row[r] = a.feat + (a.item_row0 + (live[r] ? item[r] : 0)) * a.ld;
        }
        float dot[kCandRows], ss[kCandRows];
#pragma unroll
        for (int r = 0; r < kCandRows; ++r) dot[r] = ss[r] = 0.f;
        for (int s = g; s < segs; s += G) {
            const float4 m = *reinterpret_cast<const float4*>(mrow + 4 * s);
            float4 x[kCandRows];
#pragma unroll
            for (int r = 0; r < kCandRows; ++r) x[r] = live[r] ? cand_segment(row[r], s, a.dim, vec) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
            for (int r = 0; r < kCandRows; ++r) {
                dot[r] = fmaf(x[r].x, m.x, dot[r]);
                dot[r] = fmaf(x[r].y, m.y, dot[r]);
                dot[r] = fmaf(x[r].z, m.z, dot[r]);
                dot[r] = fmaf(x[r].w, m.w, dot[r]);
                if constexpr (COSINE) {
                    ss[r] = fmaf(x[r].x, x[r].x, ss[r]);
                    ss[r] = fmaf(x[r].y, x[r].y, ss[r]);
                    ss[r] = fmaf(x[r].z, x[r].z, ss[r]);
                    ss[r] = fmaf(x[r].w, x[r].w, ss[r]);
                }
            }
        }
        for (int off = G >> 1; off >= 1; off >>= 1) {
#pragma unroll
            for (int r = 0; r < kCandRows; ++r) {
                dot[r] += __shfl_xor(dot[r], off);
                if constexpr (COSINE) ss[r] += __shfl_xor(ss[r], off);
            }
        }
        if (g == 0) {
#pragma unroll
            for (int r = 0; r < kCandRows; ++r) {
                const int e = base + r * groups + grp;
                if (e < n) {
                    float s = -__builtin_inff();
                    if (live[r]) {
                        if constexpr (COSINE) s = dot[r] / (fmaxf(sqrtf(ss[r]), kCosineEps) * norm_m) + a.bias[item[r]];
                        else s = dot[r] + a.bias[item[r]];
                    }
                    out[e] = s;
                }
            }
        }
    }
}

// a wave per search: runs[c]
__global__ __launch_bounds__(kWave) void cand_plan_kernel(const int64_t* __restrict__ cand_ptr, const int64_t* __restrict__ cand_row, int64_t n_cand_rows, int64_t total,
                                                          int64_t n_pairs, CandRun* __restrict__ runs) {
    const int lane = threadIdx.x;
    for (int64_t c = blockIdx.x; c < n_pairs; c += gridDim.x) {
        const int64_t row = cand_row != nullptr ? cand_row[c] : c;
        CandRun run{0, 0, 0};
        if (row >= 0 && row < n_cand_rows) {
            const int64_t b = cand_ptr[row], e = cand_ptr[row + 1];
            if (b >= 0 && e >= b && e <= total) {
                run.begin = b;
                run.len = static_cast<int32_t>(e - b < INT_MAX - kCandChunk ? e - b : INT_MAX - kCandChunk);
                bool named = false;                                          // by a lower-numbered search (only with cand_row: a scan of its entries below c)
                if (cand_row != nullptr)
                    for (int64_t j = lane; j < c; j += kWave) named |= cand_row[j] == row;
                run.owner = __ballot(named) == 0 ? 1 : 0;
            }
        }
        if (lane == 0) runs[c] = run;
    }
}

// one workgroup: unit_begin[c] = the scoring units of the searches below c (an owner has ceil(len / kCandChunk)), unit_begin[n_pairs] = all of them
__global__ __launch_bounds__(kBlockThreads) void cand_units_kernel(const CandRun* __restrict__ runs, int64_t n_pairs, int64_t* __restrict__ unit_begin) {
    __shared__ int64_t wave_sum[kWavesPerBlock];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int64_t carry = 0;
    for (int64_t base = 0; base < n_pairs; base += kBlockThreads) {
        const int64_t c = base + tid;
        int64_t v = 0;
        if (c < n_pairs && runs[c].owner != 0) v = (static_cast<int64_t>(runs[c].len) + kCandChunk - 1) / kCandChunk;
        int64_t incl = v;
#pragma unroll
        for (int off = 1; off < kWave; off <<= 1) {
            const int64_t o = __shfl_up(incl, off);
            if (lane >= off) incl += o;
        }
        if (lane == kWave - 1) wave_sum[wave] = incl;
        __syncthreads();
        int64_t before = carry;
        for (int w = 0; w < wave; ++w) before += wave_sum[w];
        if (c < n_pairs) unit_begin[c] = before + incl - v;
        for (int w = 0; w < kWavesPerBlock; ++w) carry += wave_sum[w];
        __syncthreads();
    }
    if (tid == 0) unit_begin[n_pairs] = carry;
}

// a wave per unit (grid-stride): the scores of chunk j of an owner's run at the run's slots
template <bool COSINE>
__global__ __launch_bounds__(kWave) void cand_score_kernel(const CandArgs a, const CandRun* __restrict__ runs, const int64_t* __restrict__ unit_begin, int64_t n_pairs,
                                                           float* __restrict__ scores) {
    __shared__ __attribute__((aligned(16))) float mrow[kCandMaxDim];
    const int64_t n_units = unit_begin[n_pairs];
    for (int64_t unit = blockIdx.x; unit < n_units; unit += gridDim.x) {
        int64_t lo = 0, hi = n_pairs;                                       // the last search whose first unit is at or before `unit` (searches without units share its value: skipped)
        while (hi - lo > 1) {
            const int64_t mid = lo + (hi - lo) / 2;
            if (unit_begin[mid] <= unit) lo = mid; else hi = mid;
        }
        const int64_t c = lo;
        const CandRun run = runs[c];
        const int e0 = static_cast<int>(unit - unit_begin[c]) * kCandChunk;
        if (run.owner == 0 || e0 >= run.len) continue;                      // (cannot happen: the scan counts exactly the owners' chunks)
        const int n = run.len - e0 < kCandChunk ? run.len - e0 : kCandChunk;
        const float norm_m = cand_mixed_row<COSINE>(a, c, mrow);
        int64_t xlo, xhi;
        cand_excl_run(a, c, xlo, xhi);
        cand_score_chunk<COSINE>(a, mrow, norm_m, a.cand_items + run.begin + e0, n, xlo, xhi, scores + run.begin + e0);
    }
}

// a wave per search (grid-stride): the ranking of its run's scores, the (-FLT_MAX, -1) tail from target = min(k, entries with a score above -inf) on, passes[c]
template <bool COSINE>
__global__ __launch_bounds__(kWave) void cand_select_kernel(const CandArgs a, const CandRun* __restrict__ runs, int64_t n_pairs, const float* __restrict__ scores, int k,
                                                            float* __restrict__ out_val, int32_t* __restrict__ out_idx, int32_t* __restrict__ passes) {
    __shared__ __attribute__((aligned(16))) float mrow[kCandMaxDim];
    __shared__ float stage[kCandChunk];
    const int lane = threadIdx.x;
    for (int64_t c = blockIdx.x; c < n_pairs; c += gridDim.x) {
        const CandRun run = runs[c];
        const bool stored = run.owner != 0;
        float norm_m = 1.f;
        int64_t xlo = 0, xhi = 0;
        if (!stored && run.len > 0) {
            norm_m = cand_mixed_row<COSINE>(a, c, mrow);
            cand_excl_run(a, c, xlo, xhi);
        }
        const int32_t* ids = a.cand_items + run.begin;
        int count = 0, trips = 0, target = -1;
        float b_val = __builtin_inff();                                     // the boundary: the last rank emitted
        int b_idx = -1;
        while (run.len > 0) {
            TopList top;
            top.init();
            int admitted = 0;
            for (int e0 = 0; e0 < run.len; e0 += kCandChunk) {
                const int n = run.len - e0 < kCandChunk ? run.len - e0 : kCandChunk;
                const float* src = scores + run.begin + e0;
                if (!stored) {
                    __syncthreads();                                         // (the previous chunk's readers of `stage`)
                    cand_score_chunk<COSINE>(a, mrow, norm_m, ids + e0, n, xlo, xhi, stage);
                    __syncthreads();
                    src = stage;
                }
                for (int t = lane; t < n; t += kWave) {
                    const float s = src[t];
                    if (s > -__builtin_inff()) {                              // (-inf: not admitted; a NaN score is never ranked either)
                        ++admitted;
                        const int i = ids[e0 + t];
                        if (ranks_before(b_val, b_idx, s, i) && ranks_before(s, i, top.val[kTopMax - 1], top.idx[kTopMax - 1])) top.insert(s, i);
                    }
                }
            }
            if (target < 0) {
#pragma unroll
                for (int off = 32; off >= 1; off >>= 1) admitted += __shfl_xor(admitted, off);
                target = admitted < k ? admitted : k;
            }
            if (target == 0) break;
            ++trips;
            const int emit = target - count < kTopMax ? target - count : kTopMax;
            int got = 0;
            for (int j = 0; j < emit; ++j) {
                float wv = top.val[0];
                int wi = top.idx[0];
#pragma unroll
                for (int off = 32; off >= 1; off >>= 1) {
                    const float ov = __shfl_xor(wv, off);
                    const int oi = __shfl_xor(wi, off);
                    if (ranks_before(ov, oi, wv, wi)) {
                        wv = ov;
                        wi = oi;
                    }
                }
                if (wi == INT_MAX) break;                                   // (only a run that is not strictly ascending: an id counted twice is ranked once)
                if (lane == 0) {
                    out_val[c * k + count] = wv;
                    out_idx[c * k + count] = wi;
                }
                if (top.idx[0] == wi) top.pop();
                ++count;
                ++got;
                b_val = wv;
                b_idx = wi;
            }
            if (count >= target || got == 0) break;
        }
        for (int t = count + lane; t < k; t += kWave) {
            out_val[c * k + t] = -FLT_MAX;
            out_idx[c * k + t] = -1;
        }
        if (lane == 0 && passes != nullptr) passes[c] = trips;
    }
}

__global__ __launch_bounds__(kBlockThreads) void cand_fill_kernel(float* __restrict__ p, int64_t n, float v) {
    for (int64_t i = static_cast<int64_t>(blockIdx.x) * kBlockThreads + threadIdx.x; i < n; i += static_cast<int64_t>(gridDim.x) * kBlockThreads) p[i] = v;
}

inline int cand_grid(int64_t waves) { return static_cast<int>(std::max<int64_t>(1, std::min<int64_t>(waves, kCandMaxGrid))); }

// The workspace, region after region: the scores of the list entries, float32 [total] | unit_begin, int64 [n_pairs + 1] (each rounded up to 16 bytes) |
// runs, CandRun [n_pairs].  A null base answers the size query (`bytes`), the caller's pointer carves the regions.
struct CandWorkspace {
    float* scores;
    int64_t* unit_begin;
    CandRun* runs;
    int64_t bytes;
};
inline CandWorkspace cand_workspace(void* base, int64_t n_pairs, int64_t total) {
    WorkspaceCursor ws(base);
    CandWorkspace w{};
    w.scores = static_cast<float*>(ws.take(align16(total * 4)));
    w.unit_begin = static_cast<int64_t*>(ws.take(align16((n_pairs + 1) * 8)));
    w.runs = static_cast<CandRun*>(ws.take(n_pairs * static_cast<int64_t>(sizeof(CandRun))));
    w.bytes = ws.at;
    return w;
}

constexpr RankRules kSearchCandidates{"ihg_search_candidates", kCandMaxK, "1 <= ", true, kCandMaxDim, "is beyond the mixed row's storage", IHG_ERR_INVALID};

// the kernels' argument block, from the record
inline CandArgs cand_args(const RankCall& c, const int32_t* cand_items) {
    CandArgs a;
    a.feat = c.features, a.ld = c.ld, a.dim = c.dim, a.query_row0 = c.query_row0, a.item_row0 = c.item_row0, a.n_items = c.n_items, a.bias = c.item_bias;
    a.group = cand_group_width(c.dim);
    a.vec = (aligned16(c.features) && c.ld % 4 == 0) ? 1 : 0;
    a.users = c.users, a.queries = c.queries, a.query_rows = c.query_rows, a.ld_q = c.ld_q, a.q_dim = c.q_dim, a.item_mask = c.item_mask;
    a.excl_ptr = c.excl_ptr, a.excl_items = c.excl_items, a.excl_row = c.excl_row, a.n_excl_rows = c.n_excl_rows;
    a.cand_items = cand_items, a.lam = c.lambda_muq;
    return a;
}

}  // namespace

extern "C" {

int32_t ihg_search_candidates_max_dim(void) { return kCandMaxDim; }

// regions: scores [total] | unit_begin [n_pairs + 1] | runs [n_pairs]
int64_t ihg_search_candidates_workspace_bytes(int64_t n_pairs, int64_t total, int32_t dim, int32_t k) {
    if (n_pairs <= 0 || total < 0 || dim <= 0 || dim > kCandMaxDim || k <= 0 || k > kCandMaxK) return 0;
    return cand_workspace(nullptr, n_pairs, total).bytes;
}

int ihg_search_candidates(const float* features, int64_t ld, int32_t dim, int64_t query_row0, int64_t item_row0, int64_t n_items, const float* item_bias,
                          const int64_t* users, const int64_t* queries, const float* query_rows, int64_t ld_q, int32_t q_dim, const uint32_t* item_mask,
                          const int64_t* excl_ptr, const int32_t* excl_items, const int64_t* excl_row, int64_t n_excl_rows, const int64_t* cand_ptr,
                          const int32_t* cand_items, const int64_t* cand_row, int64_t n_cand_rows, int64_t total, float lambda_muq, int64_t n_pairs, int32_t k,
                          float* top_scores, int32_t* top_items, float* all_scores, void* workspace, int64_t workspace_bytes, int32_t cosine, int32_t* passes,
                          ihg_stream_t stream) {
    RankCall c;
    c.features = features, c.ld = ld, c.dim = dim, c.query_row0 = query_row0, c.item_row0 = item_row0, c.n_items = n_items, c.item_bias = item_bias;
    c.users = users, c.queries = queries, c.query_rows = query_rows, c.ld_q = ld_q, c.q_dim = q_dim, c.item_mask = item_mask;
    c.excl_ptr = excl_ptr, c.excl_items = excl_items, c.excl_row = excl_row, c.n_excl_rows = n_excl_rows;
    c.lambda_muq = lambda_muq, c.n_pairs = n_pairs, c.k = k, c.top_scores = top_scores, c.top_items = top_items;
    c.workspace = workspace, c.workspace_bytes = workspace_bytes, c.cosine = cosine, c.passes = passes, c.stream = stream;
    if (int rc = rank_check_call(c, kSearchCandidates)) return rc;
    if (total < 0 || (n_pairs > 0 && (n_cand_rows < 1 || (cand_row == nullptr && n_cand_rows != n_pairs))))
        return fail(IHG_ERR_INVALID, "%s: total >= 0, n_cand_rows >= 1, and == n_pairs without cand_row", kSearchCandidates.what);
    if (n_pairs == 0) return IHG_OK;
    if (int rc = rank_check_pointers(c, kSearchCandidates, cand_ptr != nullptr && (cand_items != nullptr || total == 0))) return rc;
    if (int rc = rank_check_workspace(c, kSearchCandidates, cand_workspace(nullptr, n_pairs, total).bytes)) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const CandWorkspace ws = cand_workspace(workspace, n_pairs, total);
    float* scores = all_scores != nullptr ? all_scores : ws.scores;
    const CandArgs a = cand_args(c, cand_items);
    if (all_scores != nullptr && cand_row != nullptr && total > 0)           // a run that no search names keeps -inf: every slot is written
        hipLaunchKernelGGL(cand_fill_kernel, dim3(static_cast<unsigned>(std::min<int64_t>((total + kBlockThreads - 1) / kBlockThreads, kMaxBlocks))), dim3(kBlockThreads), 0, s,
                           all_scores, total, -__builtin_inff());
    hipLaunchKernelGGL(cand_plan_kernel, dim3(cand_grid(n_pairs)), dim3(kWave), 0, s, cand_ptr, cand_row, n_cand_rows, total, n_pairs, ws.runs);
    hipLaunchKernelGGL(cand_units_kernel, dim3(1), dim3(kBlockThreads), 0, s, ws.runs, n_pairs, ws.unit_begin);
    const int score_grid = cand_grid(total / kCandChunk + n_pairs);          // (the units are at most this many; the kernel reads their number on the device)
    if (cosine != 0) {
        hipLaunchKernelGGL(cand_score_kernel<true>, dim3(score_grid), dim3(kWave), 0, s, a, ws.runs, ws.unit_begin, n_pairs, scores);
        hipLaunchKernelGGL(cand_select_kernel<true>, dim3(cand_grid(n_pairs)), dim3(kWave), 0, s, a, ws.runs, n_pairs, scores, k, top_scores, top_items, passes);
    } else {
        hipLaunchKernelGGL(cand_score_kernel<false>, dim3(score_grid), dim3(kWave), 0, s, a, ws.runs, ws.unit_begin, n_pairs, scores);
        hipLaunchKernelGGL(cand_select_kernel<false>, dim3(cand_grid(n_pairs)), dim3(kWave), 0, s, a, ws.runs, n_pairs, scores, k, top_scores, top_items, passes);
    }
    return check_launch(kSearchCandidates.what);
}

}  // extern "C"
