// Copies between the fp32 LDS tile of a workgroup-per-tile layer kernel (layer.hip, layer_split.hip: 256 threads, 32 points x 128
// channels, LD floats per row) and global memory: rows, and the attention's fp16 hi / lo operand streams (split_layout.h).
#pragma once
#include "pdsc_common.h"
#include "split_layout.h"

namespace pdsc {

// coalesced copy of the tile to row-major global memory (ld floats per row), full 512-B rows
template <int LD>
__device__ __forceinline__ void tile_to_global(const float* Xs, float* __restrict__ dst, long long ld, int m0, int M, int t) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int f = t + 256 * i, row = f >> 5, c4 = f & 31;
        if (m0 + row < M)
            *reinterpret_cast<f32x4*>(dst + (size_t)(m0 + row) * ld + 4 * c4) = *reinterpret_cast<const f32x4*>(Xs + row * LD + 4 * c4);
    }
}

// the tile (one of q / k / v for 32 points = one key tile) -> fp16 hi/lo streams.
// WHICH: 0 = q rows, 1 = K image, 2 = V^T image.  `valid` = number of real points in the tile (the rest is zero).
// rmax: the thread's running maximum of the fp16 range sentinel (pdsc_common.h); every value converted here is noted in it.
template <int WHICH, int LD>
__device__ __forceinline__ void tile_to_split(const float* Xs, sp16* __restrict__ qrows, unsigned char* __restrict__ img,
                                              int valid, int t, float& rmax) {
    if (WHICH == 0) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int f = t + 256 * i, row = f >> 5, c4 = (f & 31) * 4;
            if (row < valid) {
                f32x4 v = *reinterpret_cast<const f32x4*>(Xs + row * LD + c4);
                range_note(rmax, v);
                sp16x4 hi, lo;
#pragma unroll
                for (int e = 0; e < 4; ++e) { sp16 x, y; split_sp16(v[e], x, y); hi[e] = x; lo[e] = y; }
                sp16* dst = qrows + (size_t)row * SPL_Q_LD + c4;
                *reinterpret_cast<sp16x4*>(dst) = hi;
                *reinterpret_cast<sp16x4*>(dst + PDSC_CHANNELS) = lo;
            }
        }
    } else if (WHICH == 1) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int f = t + 256 * i, key = f >> 4, chunk = f & 15;
            const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
            f32x4 v[2];
#pragma unroll
            for (int j = 0; j < 2; ++j) v[j] = key < valid ? *reinterpret_cast<const f32x4*>(Xs + key * LD + 8 * chunk + 4 * j) : zero;
#pragma unroll
            for (int j = 0; j < 2; ++j) range_note(rmax, v[j]);
            sp16x8 hi, lo;
#pragma unroll
            for (int e = 0; e < 8; ++e) { sp16 x, y; split_sp16(v[e >> 2][e & 3], x, y); hi[e] = x; lo[e] = y; }
            *reinterpret_cast<sp16x8*>(img + SPL_KH + spl_k_offset(key, chunk)) = hi;
            *reinterpret_cast<sp16x8*>(img + SPL_KL + spl_k_offset(key, chunk)) = lo;
        }
    } else {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int f = t + 256 * i, ch = f & 127, jh = f >> 7;
            sp16x8 hi, lo;
            float v[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const int key = spl_v_key(jh, e);
                v[e] = key < valid ? Xs[key * LD + ch] : 0.f;
            }
#pragma unroll
            for (int e = 0; e < 8; e += 2) range_note(rmax, v[e], v[e + 1]);
#pragma unroll
            for (int e = 0; e < 8; ++e) { sp16 x, y; split_sp16(v[e], x, y); hi[e] = x; lo[e] = y; }
            *reinterpret_cast<sp16x8*>(img + SPL_VH + spl_v_offset(ch, jh)) = hi;
            *reinterpret_cast<sp16x8*>(img + SPL_VL + spl_v_offset(ch, jh)) = lo;
        }
    }
}
// ... outside a forward's sentinel (layer_split.hip, experiments builds)
template <int WHICH, int LD>
__device__ __forceinline__ void tile_to_split(const float* Xs, sp16* __restrict__ qrows, unsigned char* __restrict__ img,
                                              int valid, int t) {
    float unused = 0.f;
    tile_to_split<WHICH, LD>(Xs, qrows, img, valid, t, unused);
}

}  // namespace pdsc
