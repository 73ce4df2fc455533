// f-2 / f-19: the tile body of the descriptor matcher -- ONE copy, included by match.hip (one pair per call) and match_batch.hip
// (a work list of pairs over a pool of clouds).  Both kernels call match_tile<MODE> with a source tile and a target range, so the
// distance (or inner product) of a (source, target) pair is the same bits whichever kernel computed it: the same
// v_mfma_f32_32x32x2f32 sequence in the same k order, the same sqrt_rn radicand expression, the same key order.
//   distance   = sqrt(2 - 2 * (src_desc @ tgt_desc.T) + 1e-6)   (datasets/ThreeDMatch.py:283), MODE 1: the inner product itself
//   keys[i]    = min over the target range of (distance bits << 32 | target index), merged across workgroups by one 64-bit atomicMin
// Orientation D^T = T . S^T (A = 32 target descriptors from LDS, B = 32 source descriptors held in registers) leaves the accumulator
// lane = one source point and its 16 registers = 16 targets, so the arg-min is a lane-local scan in ascending target order.
#pragma once
#include "pdsc_common.h"

namespace pdsc {

constexpr int MT_SRC = 128;      // source points per workgroup (32 per wave)
constexpr int MT_TGT = 128;      // target rows staged per barrier
constexpr int MT_MAXD = 64;      // descriptor length limit (FCGF 32, FPFH 33)

__device__ __forceinline__ unsigned long long match_key(float dist, int idx) {
    const unsigned int bits = (dist != dist) ? 0u : __float_as_uint(dist);      // dist >= 0 or NaN; NaN sorts first
    return ((unsigned long long)bits << 32) | (unsigned int)idx;
}

// MODE 1 (evaluation/test_3DLoMatch.py:45-46): source_idx = argmax_j <src_i, tgt_j> -- torch.argmax: first index among equal
// maxima, NaN counts as the maximum.  The key orders LARGER inner products first: bits = ~monotone(dot), NaN -> 0.
__device__ __forceinline__ unsigned int ip_bits(float dot) {
    if (dot != dot) return 0u;
    const unsigned int u = __float_as_uint(dot + 0.0f);                 // -0 -> +0 (equal for argmax)
    const unsigned int mono = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    return ~mono;                                                        // 0 only for mono = 0xFFFFFFFF, a NaN pattern: reserved for NaN above
}
__device__ __forceinline__ float ip_from_bits(unsigned int bits) {
    const unsigned int mono = ~bits;
    return __uint_as_float((mono & 0x80000000u) ? (mono & 0x7fffffffu) : ~mono);
}

// One workgroup of 256 threads: keys[i] = min(keys[i], min over j in [j_begin, j_end) of key(distance(i, j), j)) for the MT_SRC source
// rows from s_tile0 (rows >= Ns are computed on a clamped row and not written).  src [Ns][D], tgt [>= j_end][D], keys [>= Ns]
// pre-filled with all ones.  j_begin < j_end, both uniform over the workgroup (the body holds barriers).
template <int MODE>
__device__ __forceinline__ void match_tile(const float* __restrict__ src, const float* __restrict__ tgt, int Ns, int D, int s_tile0,
                                           int j_begin, int j_end, unsigned long long* __restrict__ keys) {
    constexpr int KP = MT_MAXD;                      // descriptor columns held (zero padded)
    constexpr int LD = KP + 4;                       // LDS row stride in floats (16-B aligned, rotates bank slots)
    __shared__ __attribute__((aligned(16))) float Ts[MT_TGT * LD];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int l31 = lane & 31, h = lane >> 5;
    const int s0 = s_tile0 + wave * 32;
    const int nq = (D + 7) / 8;                      // 8-column groups in use

    // this lane's source descriptor fragment: k-slot (4q+e, half h) <-> column 8q+4h+e
    f32x4 sf[KP / 8];
    {
        const int srow = min(s0 + l31, Ns - 1);
#pragma unroll
        for (int q = 0; q < KP / 8; ++q) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int c = 8 * q + 4 * h + e;
                sf[q][e] = c < D ? src[(size_t)srow * D + c] : 0.f;
            }
        }
    }
    float best = MODE == 0 ? INFINITY : -INFINITY;
    int best_j = 0x7fffffff;
    bool best_nan = false;

    // staging: descriptor lengths that are multiples of 4 (FCGF: 32) move as 16-byte pieces, 4 per thread and tile (r05: the
    // scalar loop below -- 32 dependent 4-byte loads per thread and tile, half of them zero fill -- was the other half of this
    // kernel's time); the columns past D that the last 8-column group reads are zeroed once
    const bool vec4 = (D & 3) == 0 && (reinterpret_cast<size_t>(tgt) & 15) == 0;
    if (vec4) {
        for (int idx = t; idx < MT_TGT * LD; idx += 256) Ts[idx] = 0.f;
    }
    for (int j0 = j_begin; j0 < j_end; j0 += MT_TGT) {
        __syncthreads();                             // previous tile consumed (first pass: the zero fill done)
        if (vec4) {
            const int c4n = D >> 2;
            for (int idx = t; idx < MT_TGT * c4n; idx += 256) {
                const int r = idx / c4n, c4 = idx - r * c4n;
                const int j = j0 + r;
                const f32x4 v = j < j_end ? *reinterpret_cast<const f32x4*>(tgt + (size_t)j * D + 4 * c4) : f32x4{0.f, 0.f, 0.f, 0.f};
                *reinterpret_cast<f32x4*>(Ts + r * LD + 4 * c4) = v;
            }
        } else {
            for (int idx = t; idx < MT_TGT * KP; idx += 256) {
                const int r = idx / KP, c = idx - r * KP;
                const int j = j0 + r;
                Ts[r * LD + c] = (j < j_end && c < D) ? tgt[(size_t)j * D + c] : 0.f;
            }
        }
        __syncthreads();
#pragma unroll
        for (int sub = 0; sub < MT_TGT / 32; ++sub) {
            if (j0 + 32 * sub >= j_end) break;       // wave-uniform
            f32x16 acc;
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = 0.f;
            const float* trow = Ts + (32 * sub + l31) * LD + 4 * h;
            for (int q = 0; q < nq; ++q) {
                const f32x4 tf = *reinterpret_cast<const f32x4*>(trow + 8 * q);
#pragma unroll
                for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(tf[e], sf[q][e], acc, 0, 0, 0);
            }
            // lane = source point l31; register r = target j0 + 32 sub + (r&3) + 8 (r>>2) + 4 h.  Ascending target order
            // within a lane is r = 0..15; the other half of the targets lives in lane + 32 (merged at the end).
            // r05: the launch is bound by this vector work, not by its 16 MFMAs per block.  MODE 0: the correctly rounded square root
            // without the library call's special-case scaffolding (sqrt_rn, pdsc_common.h: v_sqrt_f32 + the one-ulp residual test hipcc
            // itself emits; radicands here are 1e-6 .. 4, or negative / NaN -> NaN like sqrtf), and a branch-free update: a NaN
            // distance becomes -inf, which nothing beats afterwards (np.argmin: the first NaN wins) and is mapped back at the end.
            // (Measured and dropped, profiles/r05_c_match_bench_radicand_branch.txt: comparing radicands and taking the square root
            //  only on a new minimum -- with ~250 targets per workgroup some lane of the wave has a new minimum in nearly every step.)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int j = j0 + 32 * sub + (r & 3) + 8 * (r >> 2) + 4 * h;
                if (MODE == 0) {
                    float d = sqrt_rn((2.0f - 2.0f * acc[r]) + 1e-6f);                                  // reference arithmetic, fp32
                    d = d != d ? -INFINITY : d;
                    // strict: the first index among equal distances; the FIRST candidate of a lane is always taken (a row whose
                    // distances are all +inf must still return np.argmin's answer, index 0 -- with `d < best` alone no lane ever wrote a key)
                    const bool take = j < j_end && (d < best || best_j == 0x7fffffff);
                    best = take ? d : best;
                    best_j = take ? j : best_j;
                } else {
                    const float d = acc[r];
                    const bool dn = d != d;
                    const bool take = j < j_end && !best_nan && (dn || d > best || (d == best && j < best_j));
                    if (take) { best = d; best_j = j; best_nan = dn; }
                }
            }
        }
    }
    // merge the two halves of the targets, then the splits
    if (MODE == 0) best_nan = best == -INFINITY;
    unsigned long long key = MODE == 0 ? match_key(best_nan ? NAN : best, best_j)
                                       : (((unsigned long long)ip_bits(best_nan ? NAN : best) << 32) | (unsigned int)best_j);
    const unsigned long long other = __shfl_xor(key, 32, 64);
    key = other < key ? other : key;
    if (h == 0 && s0 + l31 < Ns && best_j != 0x7fffffff) atomicMin(keys + s0 + l31, key);
}

// the split rule of both launchers: the targets are cut so that ~1024 workgroups exist, in whole staged tiles.  src_tiles: source
// tiles of the launch (one pair: ceil(Ns / MT_SRC); a work list: its tile total), Nt: the (longest) target count; want > 0 overrides
// the fill rule.  Returns the targets per split; *splits = ceil(Nt / that).
static inline int match_split_plan(int src_tiles, int Nt, int want, int* splits) {
    int s = want > 0 ? want : ceil_div(1024, src_tiles);
    const int max_splits = ceil_div(Nt, MT_TGT);
    if (s > max_splits) s = max_splits;
    const int per = ceil_div(ceil_div(Nt, s), MT_TGT) * MT_TGT;
    *splits = ceil_div(Nt, per);
    return per;
}

}  // namespace pdsc
