// worklist.hpp - the work list of K7 and of every kernel that walks a graph the way K7 does (aggregate.hip: K7 itself and the pair sums; gat.hip, phase2.hip: the
// attention passes): first the fixed-length segments of the split (heavy) rows, then the light rows in `row_order`.  One description of the list (Plan), one way to
// read a unit of it on the device (unit_at), the lane-group dispatch of the launches (with_row_lanes), and the host-side construction and check of the split rows.
#pragma once
#include <type_traits>

#include "common.hpp"

namespace {

template <int G>
__device__ __forceinline__ int wave_max_len(int v) {
#pragma unroll
    for (int o = kWave / 2; o >= G; o >>= 1) {
        const int other = __shfl_xor(v, o);
        v = other > v ? other : v;
    }
    return v;
}

// The work list of K7 (aggregate.hip): first the segments of the split rows, then the light rows in `row_order`.
struct Plan {
    const int32_t* rowptr;
    const int32_t* ids;
    const int32_t* mirror;
    const int32_t* row_order;
    int64_t n_rows;
    int heavy_threshold;
    const int32_t* seg_begin;
    const int32_t* seg_end;
    const int32_t* seg_row;
    int64_t n_segments;
    const int32_t* heavy_rows;
    const int32_t* heavy_segptr;
    int64_t n_heavy;
};

// seg >= 0: a segment of a split row (its partial goes to slot seg; row = the owner).  seg < 0: a whole light row; row < 0 with len 0: nothing
// (past the end, or a split row met in the row list - its segments cover it)
struct Unit {
    int begin, len;
    int64_t row, seg;
};

__device__ __forceinline__ Unit unit_at(const Plan& pl, int64_t u) {
    Unit r{0, 0, -1, -1};
    if (u < pl.n_segments) {
        r.begin = pl.seg_begin[u];
        r.len = pl.seg_end[u] - r.begin;
        r.row = pl.seg_row[u];
        r.seg = u;
    } else if (u < pl.n_segments + pl.n_rows) {
        int64_t v = u - pl.n_segments;
        if (pl.row_order != nullptr) v = pl.row_order[v];
        r.begin = pl.rowptr[v];
        r.len = pl.rowptr[v + 1] - r.begin;
        if (pl.heavy_threshold > 0 && r.len > pl.heavy_threshold) r.len = 0;
        else r.row = v;
    }
    return r;
}

// workgroups of a split-row finish: one per split row
inline int heavy_grid(int64_t n_heavy) { return static_cast<int>(std::max<int64_t>(1, std::min<int64_t>(n_heavy, kMaxBlocks * 4))); }

// rows of `dim` floats at stride ld from p can be read 16 bytes at a time
inline bool rows16(int32_t dim, int64_t ld, const void* p) { return dim % 4 == 0 && ld % 4 == 0 && aligned16(p); }

// f(VEC, G) with both as compile-time values (std::integral_constant): VEC = 4 floats per lane where the caller found the rows 16-byte addressable, else 1;
// G = the lanes that own a row, the smallest power of two >= dim / VEC clamped to [4, 64] (K7's lane groups)
template <class F>
void with_row_lanes(bool vec4, int dim, F f) {
    const auto lanes = [&](auto vec) {
        int g = 4;
        while (g < dim / vec() && g < kWave) g <<= 1;
        switch (g) {
            case 4: f(vec, std::integral_constant<int, 4>{}); break;
            case 8: f(vec, std::integral_constant<int, 8>{}); break;
            case 16: f(vec, std::integral_constant<int, 16>{}); break;
            case 32: f(vec, std::integral_constant<int, 32>{}); break;
            default: f(vec, std::integral_constant<int, 64>{}); break;
        }
    };
    if (vec4) lanes(std::integral_constant<int, 4>{});
    else lanes(std::integral_constant<int, 1>{});
}

// a plan without split rows has no segments and no threshold, whatever the caller passed for them
Plan make_plan(const int32_t* rowptr, const int32_t* ids, const int32_t* mirror, const int32_t* row_order, int64_t n_rows, int32_t heavy_threshold,
               const int32_t* seg_begin, const int32_t* seg_end, const int32_t* seg_row, int64_t n_segments, const int32_t* heavy_rows,
               const int32_t* heavy_segptr, int64_t n_heavy) {
    Plan pl{rowptr, ids, mirror, row_order, n_rows, heavy_threshold, seg_begin, seg_end, seg_row, n_segments, heavy_rows, heavy_segptr, n_heavy};
    if (n_heavy == 0) {
        pl.n_segments = 0;
        pl.heavy_threshold = 0;
    }
    return pl;
}

// a plan with split rows names all of them (`what`: the entry point's name, as its messages carry it).  with_seg_row: the kernels read seg_row through unit_at
// (the attention passes); K7 and the pair sums resolve their units without it and leave it null
int check_split_rows(const char* what, const Plan& pl, bool with_seg_row) {
    if (pl.n_heavy > 0 && (pl.heavy_threshold <= 0 || pl.seg_begin == nullptr || pl.seg_end == nullptr || (with_seg_row && pl.seg_row == nullptr) ||
                           pl.heavy_rows == nullptr || pl.heavy_segptr == nullptr))
        return fail(IHG_ERR_INVALID, "%s: incomplete split-row plan", what);
    return IHG_OK;
}

}  // namespace
