// ranking.hpp - what the two ranking translation units share (eval.hip: the whole-catalogue entry points, candidates.hip: the shortlists): the rank order and the
// per-lane list of ten on the device; on the host the call record every extern "C" ranking function fills, the front that checks it, and the cursor their
// workspace layout functions are written with.
#pragma once
#include "common.hpp"

#include <cfloat>
#include <climits>

namespace {

constexpr int kTopMax = 10;                 // list length kept per lane (Metrics.py:60: top 10), ranks emitted per pass / trip
constexpr float kCosineEps = 1e-8f;         // torch.cosine_similarity's clamp of a norm (PredictionLayers.py:38-40)

__device__ __forceinline__ bool ranks_before(float s, int i, float v, int j) { return s > v || (s == v && i < j); }

struct TopList {
    float val[kTopMax];
    int idx[kTopMax];
    __device__ void init() {
#pragma unroll
        for (int p = 0; p < kTopMax; ++p) {
            val[p] = -FLT_MAX;
            idx[p] = INT_MAX;
        }
    }
    // sorted insert (best first); the caller has checked that (s, i) ranks before the last slot
    __device__ void insert(float s, int i) {
        val[kTopMax - 1] = s;
        idx[kTopMax - 1] = i;
#pragma unroll
        for (int p = kTopMax - 1; p > 0; --p) {
            const bool up = ranks_before(val[p], idx[p], val[p - 1], idx[p - 1]);
            const float v0 = val[p - 1], v1 = val[p];
            const int i0 = idx[p - 1], i1 = idx[p];
            val[p - 1] = up ? v1 : v0;
            val[p] = up ? v0 : v1;
            idx[p - 1] = up ? i1 : i0;
            idx[p] = up ? i0 : i1;
        }
    }
    // drop the head (statically indexed: no scratch)
    __device__ void pop() {
#pragma unroll
        for (int p = 0; p + 1 < kTopMax; ++p) {
            val[p] = val[p + 1];
            idx[p] = idx[p + 1];
        }
        val[kTopMax - 1] = -FLT_MAX;
        idx[kTopMax - 1] = INT_MAX;
    }
};

// ------------------------------------------------------------------------------------------------
// Host side.  RankCall holds what the ranking entry points have in common, in the header's words; an entry fills the fields it has and leaves the rest at "absent".
// The launch code reads the record; the kernels never see it (they keep their own argument blocks).
// ------------------------------------------------------------------------------------------------
struct RankCall {
    const float* features = nullptr;        // the score head: [N, dim] rows of stride ld, the queries' and items' first rows, the items' bias
    int64_t ld = 0, query_row0 = 0, item_row0 = 0, n_items = 0;
    int32_t dim = 0;
    const float* item_bias = nullptr;
    const int64_t *users = nullptr, *queries = nullptr;                      // the pairs; a search entry takes query_rows [n_pairs, q_dim] (stride ld_q) in place of queries
    const float* query_rows = nullptr;
    int64_t ld_q = 0;
    int32_t q_dim = 0;
    const uint32_t* item_mask = nullptr;
    const int64_t *excl_ptr = nullptr, *excl_row = nullptr;                  // the exclusion CSR, its row vector and row count
    const int32_t* excl_items = nullptr;
    int64_t n_excl_rows = 0;
    float lambda_muq = 0.f;
    int64_t n_pairs = 0;
    int32_t k = 0, cosine = 0;
    float* top_scores = nullptr;
    int32_t *top_items = nullptr, *passes = nullptr;
    void* workspace = nullptr;
    int64_t workspace_bytes = 0;
    ihg_stream_t stream = nullptr;
};

// What differs from entry to entry in the front below.
struct RankRules {
    const char* what;                       // the entry's name: every message begins with it
    int max_k;
    const char* k_from;                     // how the size message words the range: "(<k_from>k <= <max_k>)"
    bool external_queries;                  // the entry takes query_rows: exactly one query source; otherwise `queries` is one of the pointers that must be there
    int max_dim;
    const char* too_wide;                   // "feature width <dim> <too_wide> (widest: <max_dim>)"
    int short_workspace;                    // the code for a missing, misaligned or short workspace
};

// The front, in the order every entry reports in: rank_check_call, the entry's own argument rules, `n_pairs == 0` answers IHG_OK, rank_check_pointers, the entry's own
// capacity rules, rank_check_workspace.  Nothing here launches or reads device memory.
// Sizes and k; the query source; the exclusion lists (an entry without them leaves the record's fields null, which passes).
inline int rank_check_call(const RankCall& c, const RankRules& r) {
    if (c.n_pairs < 0 || c.n_items <= 0 || c.dim <= 0 || c.k <= 0 || c.k > r.max_k || c.ld < c.dim) return fail(IHG_ERR_INVALID, "%s: bad size (%sk <= %d)", r.what, r.k_from, r.max_k);
    if (r.external_queries) {
        if ((c.queries == nullptr) == (c.query_rows == nullptr)) return fail(IHG_ERR_INVALID, "%s: exactly one of queries and query_rows", r.what);
        if (c.query_rows != nullptr && (c.q_dim < 1 || c.q_dim > c.dim || c.ld_q < c.q_dim)) return fail(IHG_ERR_INVALID, "%s: 1 <= q_dim <= dim and ld_q >= q_dim", r.what);
    }
    if ((c.excl_ptr == nullptr) != (c.excl_items == nullptr)) return fail(IHG_ERR_INVALID, "%s: excl_ptr and excl_items go together", r.what);
    if (c.excl_ptr == nullptr && c.excl_row != nullptr) return fail(IHG_ERR_INVALID, "%s: excl_row without lists", r.what);
    if (c.excl_ptr != nullptr && (c.n_excl_rows < 1 || (c.excl_row == nullptr && c.n_excl_rows != c.n_pairs && c.n_pairs > 0)))
        return fail(IHG_ERR_INVALID, "%s: n_excl_rows >= 1, and == n_pairs without excl_row", r.what);
    return IHG_OK;
}

// Null pointers (`own_pointers`: those of the entry's own arguments are there), int32 item ids, the width.
inline int rank_check_pointers(const RankCall& c, const RankRules& r, bool own_pointers = true) {
    if (c.features == nullptr || c.item_bias == nullptr || c.users == nullptr || (!r.external_queries && c.queries == nullptr) || c.top_scores == nullptr ||
        c.top_items == nullptr || !own_pointers)
        return fail(IHG_ERR_INVALID, "%s: null pointer", r.what);
    if (c.n_items > INT_MAX - 64) return fail(IHG_ERR_INVALID, "%s: item ids are int32", r.what);
    if (c.dim > r.max_dim) return fail(IHG_ERR_INVALID, "%s: feature width %d %s (widest: %d)", r.what, c.dim, r.too_wide, r.max_dim);
    return IHG_OK;
}

inline int rank_check_workspace(const RankCall& c, const RankRules& r, int64_t need) {
    if (c.workspace == nullptr || !aligned16(c.workspace) || c.workspace_bytes < need) return fail(r.short_workspace, "%s: workspace too small", r.what);
    return IHG_OK;
}

// What a workspace layout function is written with: the regions one after the other, each `take` the next `bytes`.  Over a null base every region is null and `at`
// ends as the size - the layout function answers the size query and carves the caller's pointer with the same lines.
struct WorkspaceCursor {
    unsigned char* base;
    int64_t at = 0;
    explicit WorkspaceCursor(void* workspace) : base(static_cast<unsigned char*>(workspace)) {}
    void* take(int64_t bytes) {
        void* p = base != nullptr ? base + at : nullptr;
        at += bytes;
        return p;
    }
};
inline int64_t align16(int64_t n) { return (n + 15) / 16 * 16; }

}  // namespace
