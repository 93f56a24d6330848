// interact_args.hpp - what a backward call of the interactive layer wants, said once by the entry point (interact.hip) and read by every launcher of member-gradient
// kernels (interact.hip, split_arith.hip, narrow.hip): where the hyperedges' cotangents come from and whether the user slot is reduced on chip; and the two pieces every
// workspace layout is written with (Region, carve).  Host side only.
#pragma once
#include <cstdint>
#include <type_traits>

// A region of a caller's workspace as the launcher of one of its tenants gets it: where it starts (nullptr: no such region at this width) and how many floats it
// holds.  The launcher lays its image out from p with the sub-layout that stands beside its pack kernel and checks the image's end against `floats`.
struct Region { float* p; int64_t floats; };
// Float `offset` of a workspace that starts at `base`, as a T*.  base == nullptr stays nullptr: a layout function called so answers the size query.
template <typename T = float>
inline T* carve(void* base, int64_t offset) { return base != nullptr ? reinterpret_cast<T*>(static_cast<float*>(base) + offset) : nullptr; }

// [E, ld] fp32 rows of hyperedge cotangents that exist in memory (what the weight-gradient kernels read); p == nullptr: there are none
struct EdgeRows { const float* p; int64_t ld; };

// The cotangents of the hyperedges, dout [E, d], as the member-gradient kernel finds them.
struct EdgeCotangent {
    enum class Kind {
        kRows,        // src: [E, ld] fp32 rows
        kPlanes,      // src: [E][2][d] fp16 planes (ihg_edge_gather_sum_planes; d = 256, ld = d), scale: their inverse scales [E]
        kNodeLevel,   // src: the node-level cotangent [N, ld]; the kernel forms dout[e] = sum over the members m of scale[m] src[m] itself (scale == nullptr: 1)
    };
    Kind kind;
    const float* src; int64_t ld; const float* scale;
    float* store; int64_t ld_store;     // kNodeLevel: where the kernel leaves the rows it forms, [E, ld_store]; nullptr: nowhere (nobody reads them after it)

    // the fp32 rows there are once the member-gradient kernel has run: the caller's, or the ones a gathering kernel left in the store target
    EdgeRows rows_in_memory() const {
        return kind == Kind::kRows ? EdgeRows{src, ld} : (kind == Kind::kNodeLevel ? EdgeRows{store, ld_store} : EdgeRows{nullptr, 0});
    }

    static EdgeCotangent rows(const float* dout, int64_t ld) { return {Kind::kRows, dout, ld, nullptr, nullptr, 0}; }
    static EdgeCotangent planes(const void* planes_rows, int64_t dim, const float* inv_scale) { return {Kind::kPlanes, static_cast<const float*>(planes_rows), dim, inv_scale, nullptr, 0}; }
    static EdgeCotangent node_level(const float* dy, int64_t ld_dy, const float* dy_scale, float* store, int64_t ld_store) {
        return {Kind::kNodeLevel, dy, ld_dy, dy_scale, store, store != nullptr ? ld_store : 0};
    }
};

// The outputs of the user-reduced form (hyperedges numbered by user): the kernel sums the user slot on chip and writes dh[users] itself, the member buffer g is
// [E, 2, d]; runs that cross a tile range go through the boundary table (values, then their users).  A launcher that takes a pointer to this takes nullptr for
// the [E, 3, d] form.
// dp != nullptr (the gathering split kernel, where first_order_users_ok says so): the kernel also sums the cotangents it forms over each user's run - the users' rows of
// the first-order gradient, [N, ld_dp] - with the boundary runs in bnd_dp, a second value table indexed like bnd_val under the same bnd_user.
struct UserReduced { float* dh; int64_t ld_dh; float* bnd_val; int32_t* bnd_user; float* dp; int64_t ld_dp; float* bnd_dp; };

// order -> NBLK, the number of product blocks a kernel template is instantiated for (order 2: uq ui qi, order 3: and uqi): Step::run<NBLK>(call)
template <typename Step, typename Call>
auto dispatch_nblk(const Call& call) {
    return call.order == 3 ? Step::template run<4>(call) : Step::template run<3>(call);
}
// The same for a launch that is one lambda, f(std::integral_constant<int, NBLK>{}), and its sibling for the kernels templated on the order itself (2 / 3)
template <typename F>
void dispatch_nblk(int order, F&& f) {
    if (order == 3) f(std::integral_constant<int, 4>{});
    else f(std::integral_constant<int, 3>{});
}
template <typename F>
void dispatch_order(int order, F&& f) {
    if (order == 3) f(std::integral_constant<int, 3>{});
    else f(std::integral_constant<int, 2>{});
}

// The same for the node-level linear maps' launchers, which are lambdas: f(std::integral_constant<int, V>{}) with V the tiled width (32 / 64 / 128, else 256) or the
// activation of the query transform (IHG_ACT_RELU = 1, else IHG_ACT_TANH = 2); the lambda reads it back as decltype(arg)::value
template <typename F>
void dispatch_width(int dim, F&& f) {
    if (dim == 32) f(std::integral_constant<int, 32>{});
    else if (dim == 64) f(std::integral_constant<int, 64>{});
    else if (dim == 128) f(std::integral_constant<int, 128>{});
    else f(std::integral_constant<int, 256>{});
}
template <typename F>
void dispatch_act(int activation, F&& f) {
    if (activation == 1) f(std::integral_constant<int, 1>{});
    else f(std::integral_constant<int, 2>{});
}
