// One text for what decides the bits of the feature-similarity matrix (models/PointDSC.py:158-163), shared by gram_rows_kernel
// (linear.hip: pdsc_feature_compat writes M) and sm_loss_features_kernel (losses.hip: the loss of M without storing it):
// the 32 x 32 Gram tile over K = 128 channels on v_mfma_f32_32x32x2_f32 in ONE k order, and the fp32 clamp expression.
#pragma once
#include "pdsc_common.h"

namespace pdsc {

// acc[m][n] = sum over 128 channels of A[m][.] B[n][.]: one operand's fragments in registers (`reg`: this lane's row, k-slot
// (4q+e, half h) <-> channel 8q+4h+e), the other read from an LDS row (`lds_row` = row base + 4 h).  REG_IS_A: the register
// operand is the A operand (accumulator lane = the LDS row's index), else the B operand (accumulator lane = the register row).
template <bool REG_IS_A>
__device__ __forceinline__ f32x16 gram_tile_k128(const f32x4 (&reg)[16], const float* lds_row) {
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(lds_row + 8 * q);
#pragma unroll
        for (int e = 0; e < 4; ++e)
            acc = REG_IS_A ? __builtin_amdgcn_mfma_f32_32x32x2f32(reg[q][e], v[e], acc, 0, 0, 0)
                           : __builtin_amdgcn_mfma_f32_32x32x2f32(v[e], reg[q][e], acc, 0, 0, 0);
    }
    return acc;
}

// raw = 1 - (1 - <f_i, f_j>) / sigma^2 and M = clamp(raw, 0, 1), fp32, in this order of operations
__device__ __forceinline__ float feature_compat_raw(float s, float sig2) { return 1.0f - (1.0f - s) / sig2; }
__device__ __forceinline__ float feature_compat_clamp(float raw) { return fminf(fmaxf(raw, 0.0f), 1.0f); }

}  // namespace pdsc
