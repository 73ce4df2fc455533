// Merge of the attention's key-split partials for one query row: the arithmetic of attention_combine_kernel (attention.hip), used
// by the fused layer kernels so that the merge costs no launch and msg makes no round trip through HBM.  Every layer kernel merges
// with the pieces below -- the weights of a row, then one fused multiply-add chain per 4-channel piece -- so they agree bit for bit
// by construction.  The split count is a compile-time constant at every site (with_split_count): registers for exactly that many
// partials, and the loads of a batch of pieces can all be issued before any is used (a loop over a run-time count serialises
// 2 * nsplit dependent HBM round trips per piece).  What stays with each kernel is how many pieces it loads per batch
// and the addresses it loads them from (a shared address helper cost every wavefront kernel registers; the counts are at each site).
#pragma once
#include <type_traits>
#include "pdsc_common.h"

namespace pdsc {

constexpr int MERGE_MAX_SPLIT = 4;        // larger key splits go through attention_combine_kernel ...
constexpr int MERGE_MAX_SPLIT_BLOCK = 8;  // ... except in the workgroup-per-tile layer kernel (layer.hip: small problems)
constexpr int MERGE_MAX_SPLIT_H3 = 8;     // ... and in layer_h3.hip (r03: the per-GPU shares of the 8-GPU configurations -- 1-3 pairs of
                                          //     N = 5000 / 10000 -- are planned with 5-8 key splits: no combine launch, no msg round trip)

// f(std::integral_constant<int, NS>{}) with NS = the run-time split count `ns` (wave-uniform); counts of MAX and above take MAX
template <int MAX, class F>
__device__ __forceinline__ void with_split_count(int ns, F&& f) {
    static_assert(MAX == 4 || MAX == 8, "the layer kernels merge up to 4 or up to 8 splits");
    using std::integral_constant;
    if constexpr (MAX == 4) {
        switch (ns) {
            case 1: f(integral_constant<int, 1>{}); break;
            case 2: f(integral_constant<int, 2>{}); break;
            case 3: f(integral_constant<int, 3>{}); break;
            default: f(integral_constant<int, 4>{}); break;
        }
    } else {
        switch (ns) {
            case 1: f(integral_constant<int, 1>{}); break;
            case 2: f(integral_constant<int, 2>{}); break;
            case 3: f(integral_constant<int, 3>{}); break;
            case 4: f(integral_constant<int, 4>{}); break;
            case 5: f(integral_constant<int, 5>{}); break;
            case 6: f(integral_constant<int, 6>{}); break;
            case 7: f(integral_constant<int, 7>{}); break;
            default: f(integral_constant<int, 8>{}); break;
        }
    }
}

// weights of one row: w[sp] = exp2(m_sp - max m), den = sum l_sp w[sp], rden = 1 / den
template <int NS>
struct MergeWeights {
    float w[NS], den, rden;
};

// ... from the row's (m, l) pairs (the attention workgroup that merges its own leaves holds the last leaf's pair in registers)
template <int NS>
__device__ __forceinline__ MergeWeights<NS> merge_weights_of(const float2 (&ml)[NS]) {
    MergeWeights<NS> r;
    float ls[NS];
#pragma unroll
    for (int sp = 0; sp < NS; ++sp) { r.w[sp] = ml[sp].x; ls[sp] = ml[sp].y; }
    float mmax = r.w[0];
#pragma unroll
    for (int sp = 1; sp < NS; ++sp) mmax = fmaxf(mmax, r.w[sp]);
    float den = 0.f;
#pragma unroll
    for (int sp = 0; sp < NS; ++sp) {
        r.w[sp] = __builtin_amdgcn_exp2f(r.w[sp] - mmax);
        den = fmaf(ls[sp], r.w[sp], den);
    }
    r.den = den;
    r.rden = 1.0f / den;                   // one correctly-rounded reciprocal per row, then multiplies
    return r;
}
// ... loaded: slot0 = the row's slot in split 0 of its pair, sp_stride = slots per split (Npad)
template <int NS>
__device__ __forceinline__ MergeWeights<NS> merge_row_weights(const float* __restrict__ part_ml, size_t slot0, size_t sp_stride) {
    float2 ml[NS];
#pragma unroll
    for (int sp = 0; sp < NS; ++sp) ml[sp] = *reinterpret_cast<const float2*>(part_ml + (slot0 + (size_t)sp * sp_stride) * 2);
    return merge_weights_of<NS>(ml);
}

// The un-normalised sum of channel e of one 4-channel piece over its NS loaded partials, in partial order.  Two sites run it: the
// layer kernels (merge_apply below), and the attention workgroup that owns every leaf of its query block (attention_split.hip),
// which leaves the sum with (m, l) = (0, den) as the pair's ONE partial.  Merging that partial reproduces the NS-way merge bit for
// bit: w = exp2(0 - 0) = 1, den' = fmaf(den, 1, 0) = den, hence the same reciprocal, and fmaf(s, 1, 0) = s (a chain that starts
// from +0 never ends in -0), so s * rden is the same product.
template <int NS>
__device__ __forceinline__ float merge_chain(const f32x4 (&pv)[NS], const MergeWeights<NS>& mw, int e) {
    float s = 0.f;
#pragma unroll
    for (int sp = 0; sp < NS; ++sp) s = fmaf(pv[sp][e], mw.w[sp], s);
    return s;
}
// one 4-channel piece from its NS loaded partials (and channel e of it alone, for callers that pin each value as it is made)
template <int NS>
__device__ __forceinline__ float merge_apply(const f32x4 (&pv)[NS], const MergeWeights<NS>& mw, int e) {
    return merge_chain<NS>(pv, mw, e) * mw.rden;
}
template <int NS>
__device__ __forceinline__ f32x4 merge_apply(const f32x4 (&pv)[NS], const MergeWeights<NS>& mw) {
    f32x4 v;
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = merge_apply<NS>(pv, mw, e);
    return v;
}

}  // namespace pdsc
