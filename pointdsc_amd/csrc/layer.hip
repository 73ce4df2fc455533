// a-2 fused: the whole point-wise chain between two attention calls in ONE launch
//   tail of layer i   : feat  = featB + fc3( relu(fc2'( relu(fc1'(msg)) )) )         (fc_message, BN folded; reference
//                                                                                      models/PointDSC.py:43-45)
//   head of layer i+1 : featB = relu(pcn'(feat)) ; (q|k|v) = Wqkv featB + b            (models/PointDSC.py:75, :36-38)
// The five GEMMs of a 32-point tile run back to back in one 4-wave workgroup: activations never leave the
// CU (two 32x132 LDS tiles, ping-pong), each wave owns whole 32-column output tiles and reads the weight rows
// of its tile straight from L2 into registers (a weight tile is used by exactly one wave of the workgroup, so
// staging it in LDS would buy nothing), the next stage's weights are prefetched under the current stage's MFMAs.
// MFMA orientation: D = W_tile (A, rows = output channels) x X^T (B, columns = points), so the accumulator
// lane is a point and register r = 4g+e holds output channel n0+8g+4h+e: one float4 per (g) goes to LDS / HBM.
// Bound: MFMA (172 kFLOP per point per layer on v_mfma_f32_32x32x2_f32); weights stream from L2 (336 KB per tile).
#include <stdlib.h>
#include <type_traits>
#include "pdsc_common.h"
#include "split_layout.h"
#include "merge_partials.h"
#include "layer_args.h"
#include "layer_block.h"

namespace pdsc {

constexpr int LF_ROWS = 32;                  // points per workgroup
constexpr int LF_LD = PDSC_CHANNELS + 4;     // padded LDS row (floats)
constexpr int LF_TILE = LF_ROWS * LF_LD;


#define LF_STAMP(k)                                                                                   \
    if (a.trace && lane == 0) a.trace[(((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 4 + wave) * 16 + (k)] = __builtin_readcyclecounter();

template <int K>
__device__ __forceinline__ void load_w(const float* __restrict__ W, int n0, int l31, int h, f32x4 (&w)[K / 8]) {
    const float* p = W + (size_t)(n0 + l31) * K + 4 * h;
#pragma unroll
    for (int q = 0; q < K / 8; ++q) w[q] = *reinterpret_cast<const f32x4*>(p + 8 * q);
}

template <int K>
__device__ __forceinline__ void load_x(const float* Xs, int l31, int h, f32x4 (&x)[K / 8]) {
    const float* p = Xs + l31 * LF_LD + 4 * h;
#pragma unroll
    for (int q = 0; q < K / 8; ++q) x[q] = *reinterpret_cast<const f32x4*>(p + 8 * q);
}

template <int K>
__device__ __forceinline__ f32x16 mma_tile(const f32x4 (&w)[K / 8], const f32x4 (&x)[K / 8]) {
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
    for (int q = 0; q < K / 8; ++q)
#pragma unroll
        for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(w[q][e], x[q][e], acc, 0, 0, 0);
    return acc;
}

// acc -> (+bias)(relu)(+residual row from HBM) -> LDS tile Xo[point][col0 + 8g+4h .. +3]
template <bool RELU, bool RESID>
__device__ __forceinline__ void store_tile(const f32x16& acc, const float* __restrict__ bias, int n0, float* Xo, int col0,
                                           int l31, int h, const float* __restrict__ res_row) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const f32x4 bv = *reinterpret_cast<const f32x4*>(bias + n0 + 8 * g + 4 * h);
        f32x4 v;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float t = acc[4 * g + e] + bv[e];
            if (RELU) t = fmaxf(t, 0.f);
            v[e] = t;
        }
        if (RESID) {
            const f32x4 rv = *reinterpret_cast<const f32x4*>(res_row + n0 + 8 * g + 4 * h);
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = rv[e] + v[e];
        }
        *reinterpret_cast<f32x4*>(Xo + l31 * LF_LD + col0 + 8 * g + 4 * h) = v;
    }
}

// coalesced copy of row-major global memory into a 32x128 LDS tile (the other direction: layer_block.h)
__device__ __forceinline__ void global_to_tile(const float* __restrict__ src, float* Xs, int m0, int M, int t) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int f = t + 256 * i, row = f >> 5, c4 = f & 31;
        const int m = min(m0 + row, M - 1);
        *reinterpret_cast<f32x4*>(Xs + row * LF_LD + 4 * c4) = *reinterpret_cast<const f32x4*>(src + (size_t)m * PDSC_CHANNELS + 4 * c4);
    }
}

// tail input: merged msg rows, or the merge of the attention's key-split partials (merge_partials.h)
__device__ __forceinline__ void msg_to_tile(const LayerArgs& a, int b, float* Xs, int m0, int M, int t) {
    if (a.msg) {
        global_to_tile(a.msg, Xs, m0, M, t);
        return;
    }
    // 1..4 splits: the loads of all four pieces of a thread are issued before any is used (one round trip of latency).
    // 5..8 splits (small problems: the attention plan splits the keys further to fill the chip): one piece at a time --
    // registers for a single set of NS partials; costs four dependent round trips instead of one, still cheaper than the
    // attention_combine launch + the msg round trip it replaces
    with_split_count<MERGE_MAX_SPLIT_BLOCK>(a.nsplit, [&](auto ns_tag) {
        constexpr int NS = decltype(ns_tag)::value;
        constexpr int NB = NS <= 4 ? 4 : 1;                          // pieces per batch of loads
#pragma unroll
        for (int i0 = 0; i0 < 4; i0 += NB) {
            MergeWeights<NS> mw[NB];
            f32x4 pv[NB][NS];
#pragma unroll
            for (int i = 0; i < NB; ++i) {
                const int f = t + 256 * (i0 + i), row = f >> 5, c4 = (f & 31) * 4;
                const int m = min(m0 + row, M - 1);
                const size_t slot0 = (size_t)b * NS * a.Npad + (size_t)(m - b * a.N);
                mw[i] = merge_row_weights<NS>(a.part_ml, slot0, (size_t)a.Npad);
#pragma unroll
                for (int sp = 0; sp < NS; ++sp)
                    pv[i][sp] = *reinterpret_cast<const f32x4*>(a.part_o + (slot0 + (size_t)sp * a.Npad) * PDSC_CHANNELS + c4);
            }
#pragma unroll
            for (int i = 0; i < NB; ++i) {
                const int f = t + 256 * (i0 + i), row = f >> 5, c4 = (f & 31) * 4;
                *reinterpret_cast<f32x4*>(Xs + row * LF_LD + c4) = merge_apply<NS>(pv[i], mw[i]);
            }
        }
    });
}

constexpr int LF_XLD16 = PDSC_CHANNELS + 8;          // fp16 elements per row of a hi / lo activation tile (272 B)
constexpr int LF_XB_FLOATS = LF_ROWS * LF_XLD16;     // Xb doubles as the fp16 hi|lo image of featB: 2 * 32 * 136 * 2 B

template <bool HAS_TAIL, bool HAS_HEAD, bool QKV_X3>
__global__ __launch_bounds__(256, 3) void layer_fused_kernel(LayerArgs a) {
    __shared__ __attribute__((aligned(16))) float Xa[LF_TILE];
    __shared__ __attribute__((aligned(16))) float Xb[LF_XB_FLOATS > LF_TILE ? LF_XB_FLOATS : LF_TILE];
    const int t = threadIdx.x, lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int l31 = lane & 31, h = lane >> 5;
    const int m0 = blockIdx.y * a.N + blockIdx.x * LF_ROWS;     // first row of this tile
    const int M = blockIdx.y * a.N + (a.nvalid ? a.nvalid[blockIdx.y] : a.N);     // end of this pair's rows
    if (m0 >= M) return;                                         // (ragged batches: tile past the pair's own rows; workgroup-uniform)

    LF_STAMP(0)
    float rmax = 0.f;                                                // fp16 range sentinel (pdsc_common.h): what this thread converts to fp16 pairs (QKV_X3)
    f32x4 wpre[16];                                                  // PointCN weight tile of this wave (prefetched early)
    if (HAS_TAIL) {
        f32x4 w128[16], w64[8];
        // ---- fc1: 128 -> 64 (+BN, ReLU): tiles {0,1} on waves {0,1} ----
        if (wave < 2) load_w<128>(a.w1, 32 * wave, l31, h, w128);
        msg_to_tile(a, blockIdx.y, Xa, m0, M, t);
        LF_STAMP(1)
        __syncthreads();
        LF_STAMP(2)
        if (wave < 2) {
            f32x4 x[16];
            load_x<128>(Xa, l31, h, x);
            load_w<64>(a.w2, 32 * wave, l31, h, w64);                 // prefetch fc2 weights
            const f32x16 acc = mma_tile<128>(w128, x);
            store_tile<true, false>(acc, a.b1, 32 * wave, Xb, 32 * wave, l31, h, nullptr);
        }
        LF_STAMP(3)
        __syncthreads();
        // ---- fc2: 64 -> 64 (+BN, ReLU) ----
        f32x4 w3r[8];
        load_w<64>(a.w3, 32 * wave, l31, h, w3r);                     // prefetch fc3 weights (all waves)
        if (wave < 2) {
            f32x4 x[8];
            load_x<64>(Xb, l31, h, x);
            const f32x16 acc = mma_tile<64>(w64, x);
            store_tile<true, false>(acc, a.b2, 32 * wave, Xa, 32 * wave, l31, h, nullptr);
        }
        LF_STAMP(4)
        __syncthreads();
        // ---- fc3: 64 -> 128, + residual featB: tile = wave ----
        if (HAS_HEAD) load_w<128>(a.wp, 32 * wave, l31, h, wpre);      // PointCN weights of the head: under fc3's MFMAs
        {
            f32x4 x[8];
            load_x<64>(Xa, l31, h, x);
            const f32x16 acc = mma_tile<64>(w3r, x);
            const float* res_row = a.res + (size_t)min(m0 + l31, M - 1) * PDSC_CHANNELS;
            store_tile<false, true>(acc, a.b3, 32 * wave, Xb, 32 * wave, l31, h, res_row);
        }
        LF_STAMP(5)
        __syncthreads();
        LF_STAMP(6)
        if (a.feat_out) tile_to_global<LF_LD>(Xb, a.feat_out, PDSC_CHANNELS, m0, M, t);
    } else {
        if (HAS_HEAD) load_w<128>(a.wp, 32 * wave, l31, h, wpre);
        global_to_tile(a.feat_in, Xb, m0, M, t);
        __syncthreads();
    }

    if (HAS_HEAD && !QKV_X3) {
        // ---- PointCN: 128 -> 128 (+BN, ReLU): tile = wave; input Xb, output Xa ----
        f32x4 w[16], x[16];
        load_x<128>(Xb, l31, h, x);
        {
            const f32x16 acc = mma_tile<128>(wpre, x);
            load_w<128>(a.wq, 32 * wave, l31, h, w);                  // prefetch first qkv tile
            store_tile<true, false>(acc, a.bp, 32 * wave, Xa, 32 * wave, l31, h, nullptr);
        }
        __syncthreads();
        tile_to_global<LF_LD>(Xa, a.featB_out, PDSC_CHANNELS, m0, M, t);
        load_x<128>(Xa, l31, h, x);
        // ---- q|k|v: 128 -> 384 in three 128-column chunks staged through Xb ----
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int n0 = 128 * c + 32 * wave;
            const f32x16 acc = mma_tile<128>(w, x);
            if (c < 2) load_w<128>(a.wq, n0 + 128, l31, h, w);        // prefetch next chunk's tile
            store_tile<false, false>(acc, a.bq, n0, Xb, 32 * wave, l31, h, nullptr);
            __syncthreads();
            if (a.qkv_out) tile_to_global<LF_LD>(Xb, a.qkv_out + 128 * c, 3 * PDSC_CHANNELS, m0, M, t);
            if (a.qs) {      // (stage-level calls only: a forward's split attention comes with wq_split, the form below, which carries the sentinel)
                unsigned char* img = a.kv + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * SPL_TILE_STRIDE;
                const int valid = min(LF_ROWS, M - m0);
                if (c == 0) tile_to_split<0, LF_LD>(Xb, a.qs + (size_t)m0 * SPL_Q_LD, img, valid, t);
                else if (c == 1) tile_to_split<1, LF_LD>(Xb, nullptr, img, valid, t);
                else tile_to_split<2, LF_LD>(Xb, nullptr, img, valid, t);
            }
            if (c < 2) __syncthreads();
        }
    }
    if (HAS_HEAD && QKV_X3) {
        // ---- PointCN exactly as above (exact fp32: featB is the next residual) ... ----
        sp16* Xh = reinterpret_cast<sp16*>(Xb);
        sp16* Xl = Xh + LF_ROWS * LF_XLD16;
        sp16x8 wh[8], wl[8];
        {
            f32x4 x[16];
            load_x<128>(Xb, l31, h, x);
            // prefetch the first split qkv tile: lane (row l31, half h), step kk holds k = 16kk+8h..+7
            {
                const sp16* p = a.wq_split + (size_t)(32 * wave + l31) * PDSC_CHANNELS + 8 * h;
#pragma unroll
                for (int kk = 0; kk < 8; ++kk) {
                    wh[kk] = *reinterpret_cast<const sp16x8*>(p + 16 * kk);
                    wl[kk] = *reinterpret_cast<const sp16x8*>(p + (size_t)3 * PDSC_CHANNELS * PDSC_CHANNELS + 16 * kk);
                }
            }
            const f32x16 acc = mma_tile<128>(wpre, x);
            // (the first split qkv tile was requested above, under these MFMAs)
            LF_STAMP(7)
            __syncthreads();                                          // every wave holds its copy of Xb: Xb may be rewritten
            // ... stored twice: fp32 -> Xa (featB_out), fp16 hi|lo -> Xb (operand of the split-precision q|k|v GEMM)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int col = 32 * wave + 8 * g + 4 * h;
                const f32x4 bv = *reinterpret_cast<const f32x4*>(a.bp + col);
                f32x4 v;
                sp16x4 hi, lo;
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = fmaxf(acc[4 * g + e] + bv[e], 0.f);
                range_note(rmax, v);
#pragma unroll
                for (int e = 0; e < 4; ++e) { sp16 xh, xl; split_sp16(v[e], xh, xl); hi[e] = xh; lo[e] = xl; }
                *reinterpret_cast<f32x4*>(Xa + l31 * LF_LD + col) = v;
                *reinterpret_cast<sp16x4*>(Xh + l31 * LF_XLD16 + col) = hi;
                *reinterpret_cast<sp16x4*>(Xl + l31 * LF_XLD16 + col) = lo;
            }
        }
        LF_STAMP(8)
        __syncthreads();
        tile_to_global<LF_LD>(Xa, a.featB_out, PDSC_CHANNELS, m0, M, t);
        LF_STAMP(9)
        // ---- q|k|v: 128 -> 384, three 128-column chunks, hi*hi + hi*lo + lo*hi on the fp16 matrix cores, staged via Xa ----
        unsigned char* img = a.kv ? a.kv + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * SPL_TILE_STRIDE : nullptr;
        const int valid = min(LF_ROWS, M - m0);
        const int xo = l31 * LF_XLD16 + 8 * h;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int n0 = 128 * c + 32 * wave;
            const f32x16 zero = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            f32x16 acc = zero;
#pragma unroll
            for (int kk = 0; kk < 8; ++kk) {
                const sp16x8 xh = *reinterpret_cast<const sp16x8*>(Xh + xo + 16 * kk);
                const sp16x8 xl = *reinterpret_cast<const sp16x8*>(Xl + xo + 16 * kk);
                acc = PDSC_MFMA_X3(wl[kk], xh, acc, 0, 0, 0);
                acc = PDSC_MFMA_X3(wh[kk], xl, acc, 0, 0, 0);
                acc = PDSC_MFMA_X3(wh[kk], xh, acc, 0, 0, 0);
            }
            if (c < 2) {                                              // prefetch next chunk's tile
                const sp16* p = a.wq_split + (size_t)(n0 + 128 + l31) * PDSC_CHANNELS + 8 * h;
#pragma unroll
                for (int kk = 0; kk < 8; ++kk) {
                    wh[kk] = *reinterpret_cast<const sp16x8*>(p + 16 * kk);
                    wl[kk] = *reinterpret_cast<const sp16x8*>(p + (size_t)3 * PDSC_CHANNELS * PDSC_CHANNELS + 16 * kk);
                }
            }
            if (c == 0) { LF_STAMP(10) }
            __syncthreads();                                          // previous readers of Xa are done
            store_tile<false, false>(acc, a.bq, n0, Xa, 32 * wave, l31, h, nullptr);
            __syncthreads();
            if (c == 0) { LF_STAMP(11) }
            if (a.qkv_out) tile_to_global<LF_LD>(Xa, a.qkv_out + 128 * c, 3 * PDSC_CHANNELS, m0, M, t);
            if (a.qs) {
                if (c == 0) tile_to_split<0, LF_LD>(Xa, a.qs + (size_t)m0 * SPL_Q_LD, img, valid, t, rmax);
                else if (c == 1) tile_to_split<1, LF_LD>(Xa, nullptr, img, valid, t, rmax);
                else tile_to_split<2, LF_LD>(Xa, nullptr, img, valid, t, rmax);
            }
            if (c == 0) { LF_STAMP(12) }
        }
        LF_STAMP(13)
    }
    if (HAS_HEAD && QKV_X3) range_report(a.range_flag, blockIdx.y, rmax);      // once per wavefront
}

template <bool T, bool H>
static int launch_layer(const LayerArgs& a, hipStream_t st) {
    if (H && a.wq_split)
        hipLaunchKernelGGL((layer_fused_kernel<T, H, H>), dim3(ceil_div(a.N, LF_ROWS), a.bs), dim3(256), 0, st, a);
    else
        hipLaunchKernelGGL((layer_fused_kernel<T, H, false>), dim3(ceil_div(a.N, LF_ROWS), a.bs), dim3(256), 0, st, a);
    return check_launch("pdsc_layer_run(block)");
}

}  // namespace pdsc

static long long* g_layer_trace = nullptr;
long long* pdsc_layer_trace_buffer(void) { return g_layer_trace; }      // shared with layer_wave.hip
extern "C" int pdsc_layer_trace(long long* device_buffer) {       // diagnostics: see include/pointdsc_hip.h
    g_layer_trace = device_buffer;
    return PDSC_OK;
}

// Size rule, from the hipEvent-timed fused layer launch at N = 5000 (us, block / wave; tiles = pairs x 157): 2 pairs 37 / 55,
// 3 pairs (471 tiles) 43 / 61, 4 pairs (628) 56 / 53, 6 pairs (942) 70 / 56, 8 pairs 93 / 94, 16 pairs 190 / 163,
// 32 pairs 347 / 250.  Block up to two workgroups per CU.
// r02, wavefront-resident kernel with the H3 GEMMs (layer_h3.hip; whole forward, ms per step, block / wave,
// profiles/r02_j_ab_block_vs_h3.txt): N = 5000 x 1 pair (157 tiles) 1.200 / 1.235, 2 pairs (314) 1.708 / 1.664, 3 pairs (471)
// 1.985 / 1.929; N = 10000 x 1 (313) 2.682 / 2.682; N = 1000 x 1 (32) 0.572 / 0.659, x 4 (128) 0.641 / 0.712: block while the
// tiles leave CUs empty (about one workgroup per CU).
extern "C" int pdsc_layer_prefers_block(int bs, int N) {
    return (long long)bs * pdsc::ceil_div(N, pdsc::LF_ROWS) <= 288;
}

namespace pdsc {

// Every check the fused-layer entry points make, once.  The weights come as fragment streams in the H3 kernel and, in the
// wavefront kernel, when either stream is given; else in natural layout.
int validate_layer_args(const LayerArgs& a, LayerKernel kernel, const char* who) {
    const bool tail = a.msg != nullptr || a.part_o != nullptr, head = a.featB_out != nullptr;
    const bool h3 = kernel == LayerKernel::H3;
    const bool frag = h3 || (kernel == LayerKernel::Wave && (a.wf_tail || a.wf_head));
    const int io = a.io_flags;
    PDSC_REQUIRE(tail || head, "%s: neither tail (msg / partials) nor head (featB_out) requested", who);
    PDSC_REQUIRE(a.bs > 0 && a.N > 0, "%s: bs=%d N=%d", who, a.bs, a.N);
    PDSC_REQUIRE(a.gemm_format == PDSC_LAYER_GEMM_F32 || a.gemm_format == PDSC_LAYER_GEMM_H3, "%s: gemm_format=%d", who, a.gemm_format);
    PDSC_REQUIRE((io & ~(PDSC_IO_PARTIALS_PF | PDSC_IO_RES_PF | PDSC_IO_FEATB_PF)) == 0, "%s: io_flags=%d", who, io);
    PDSC_REQUIRE(h3 || (io == 0 && !a.value_fold), "%s: point-fragment hand-offs and the folded layer exist in the H3 kernel only", who);
    PDSC_REQUIRE(!h3 || a.gemm_format == PDSC_LAYER_GEMM_H3, "%s: point-fragment hand-offs need gemm_format = PDSC_LAYER_GEMM_H3", who);
    PDSC_REQUIRE(!a.value_fold || (io & PDSC_IO_PARTIALS_PF) || !tail, "%s: the folded layer merges point-fragment partials", who);
    if (tail) {
        PDSC_REQUIRE(a.res && (frag ? a.wf_tail != nullptr : a.w1 && a.b1 && a.w2 && a.b2 && a.w3 && a.b3),
                     "%s: tail needs res and fc1..fc3 (natural layout or the tail stream)", who);
        if (!a.msg) PDSC_REQUIRE(a.part_ml && a.nsplit >= 1 && a.nsplit <= layer_merge_limit(kernel) && a.Npad >= a.N,
                                 "%s: partials need part_ml, 1 <= nsplit <= %d (what this launch's kernel merges), Npad >= N", who,
                                 layer_merge_limit(kernel));
        if (!a.msg) PDSC_REQUIRE(a.part_slots == a.nsplit || (h3 && a.part_slots > a.nsplit),
                                 "%s: part_slots=%d (partials per pair in the layout) must be nsplit=%d, or more in the H3 kernels", who,
                                 a.part_slots, a.nsplit);
        PDSC_REQUIRE(!(io & PDSC_IO_PARTIALS_PF) || (!a.msg && a.Npad % 32 == 0), "%s: PF partials come un-merged (msg NULL), Npad a multiple of 32", who);
    } else {
        PDSC_REQUIRE(a.feat_in, "%s: head-only needs feat_in", who);
        PDSC_REQUIRE(!(io & (PDSC_IO_PARTIALS_PF | PDSC_IO_RES_PF)), "%s: head-only takes feat_in in row order", who);
    }
    if (head) PDSC_REQUIRE((a.qkv_out || a.qs) && (frag ? a.wf_head != nullptr : a.wp && a.bp && a.wq && a.bq),
                           "%s: head needs qkv_out or the split streams, and pcn, qkv weights (natural layout or the head stream)", who);
    else PDSC_REQUIRE(a.feat_out && !(io & PDSC_IO_FEATB_PF), "%s: tail-only needs feat_out (row order)", who);
    PDSC_REQUIRE((a.qs == nullptr) == (a.kv == nullptr), "%s: q_split and kv_tiles go together", who);
    PDSC_REQUIRE(!h3 || launch_layer_h3_fits(a, tail, head), "%s: output set not served by the H3 kernel (head: the split streams "
                 "only; tail + head: no feat_out; tail only: feat_out)", who);
    return PDSC_OK;
}

int dispatch_layer(const LayerArgs& a, LayerKernel kernel, hipStream_t st) {
    const bool tail = a.msg != nullptr || a.part_o != nullptr, head = a.featB_out != nullptr;
    if (kernel == LayerKernel::H3) {
        LayerArgs h = a;       // (the start delay is the H3 kernel's alone)
        h.stagger_cycles = env_int("PDSC_LAYER_STAGGER", 0);
        h.stagger_mode = env_int("PDSC_LAYER_STAGGER_MODE", 1);
        return launch_layer_h3(h, tail, head, st);
    }
    if (kernel == LayerKernel::Wave) return launch_layer_wave(a, tail, head, st);
    if (kernel == LayerKernel::X3) return launch_layer_x3(a, tail, head, st);
    if (tail && head) {
        profile_mark_begin(PDSC_PROF_LAYER, st);
        const int rc = launch_layer<true, true>(a, st);
        profile_mark_end(PDSC_PROF_LAYER, st);
        return rc;
    }
    if (tail) return launch_layer<true, false>(a, st);
    return launch_layer<false, true>(a, st);
}

}  // namespace pdsc

// The kernel of a pdsc_layer_run call.  PDSC_LAYER_KERNEL_AUTO:
//   natural-layout weights: two implementations.  layer_wave.hip (one wavefront per 32-point tile) wins once the tiles fill the
//     chip; with few tiles its serial 46k matrix-pipe cycles per tile are the launch time, and this file's kernel, which spreads
//     a tile over the four SIMDs of a CU, is faster (N = 1000, one pair: 0.68 vs 1.10 ms per forward).
//     (experiments builds) PDSC_LAYER_VARIANT = block | wave overrides the size rule.
//   fragment streams, point-fragment hand-offs: the H3 kernel alone reads / writes them; validate_layer_args rejects what it
//     does not serve.
//   fragment streams, plain rows: the pipelined kernel of layer_h3.hip for H3 streams and the output sets it serves, else
//     layer_wave.hip (fp32 streams, or its own H3 form); (experiments builds) A/B knob PDSC_LAYER_H3_VARIANT = 0: never H3.
// A forced kernel is taken as given: validate_layer_args rejects the arguments that do not fit it.
static bool choose_layer_kernel(const pdsc_layer_call& c, const pdsc::LayerArgs& a, pdsc::LayerKernel* kernel) {
    using pdsc::LayerKernel;
    switch (c.kernel) {
        case PDSC_LAYER_KERNEL_BLOCK: *kernel = LayerKernel::Block; return true;
        case PDSC_LAYER_KERNEL_WAVE: *kernel = LayerKernel::Wave; return true;
        case PDSC_LAYER_KERNEL_H3: *kernel = LayerKernel::H3; return true;
        case PDSC_LAYER_KERNEL_X3: *kernel = LayerKernel::X3; return true;
        case PDSC_LAYER_KERNEL_AUTO: break;
        default: return false;
    }
    if (!a.wf_tail && !a.wf_head) {
        const char* ev = pdsc::env_str("PDSC_LAYER_VARIANT");
        const bool block = ev && (ev[0] == 'b' || ev[0] == 'w') ? ev[0] == 'b' : pdsc_layer_prefers_block(c.bs, c.N) != 0;
        *kernel = block ? LayerKernel::Block : LayerKernel::Wave;
    } else if (c.io_flags != 0) {
        *kernel = LayerKernel::H3;
    } else {
        const bool h3 = c.gemm_format == PDSC_LAYER_GEMM_H3 && pdsc::env_int("PDSC_LAYER_H3_VARIANT", 1) != 0 &&
                        pdsc::launch_layer_h3_fits(a, a.msg != nullptr || a.part_o != nullptr, a.featB_out != nullptr);
        *kernel = h3 ? LayerKernel::H3 : LayerKernel::Wave;
    }
    return true;
}

extern "C" int pdsc_layer_run(const pdsc_layer_call* call, void* stream) {
    PDSC_REQUIRE(call, "pdsc_layer_run: null call");
    const pdsc_layer_call& c = *call;
    const bool natural = c.w1 || c.b1 || c.w2 || c.b2 || c.w3 || c.b3 || c.wp || c.bp || c.wq || c.bq || c.wq_split;
    PDSC_REQUIRE(!natural || (!c.wfrag_tail && !c.wfrag_head), "pdsc_layer_run: weights given in natural layout AND as fragment streams");
    if (c.featB_out && !c.q_split && !c.kv_tiles) PDSC_REQUIRE(c.qkv_out, "pdsc_layer_run: head needs qkv_out when no split streams are given");
    pdsc::LayerArgs a = pdsc::layer_args_from_call(c);
    a.trace = c.io_flags ? nullptr : g_layer_trace;      // (the point-fragment route takes no trace: layer_args.h)
    pdsc::LayerKernel kernel;
    PDSC_REQUIRE(choose_layer_kernel(c, a, &kernel), "pdsc_layer_run: kernel=%d", c.kernel);
    const int rc = pdsc::validate_layer_args(a, kernel, "pdsc_layer_run");
    return rc != PDSC_OK ? rc : pdsc::dispatch_layer(a, kernel, (hipStream_t)stream);
}
