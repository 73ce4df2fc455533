// Building blocks of the wavefront-resident fused layer kernel (layer_wave.hip): weight-chunk streams, MFMA steps,
// fp16 hi/lo splitting, the wave-private LDS patch.
#pragma once
#include <type_traits>
#include "pdsc_common.h"
#include "split_layout.h"
#include "merge_partials.h"
#include "layer_args.h"

namespace pdsc {

constexpr int LW_WAVES = 4;      // independent wavefronts per workgroup
constexpr int LW_VLD = 36;       // floats per key row of the V transpose patch (32 channels + 4 pad)
constexpr int LW_QKV_BUFS = 4;   // weight-chunk buffers (32 registers each) during the split q|k|v projection
#ifndef LW_H3_BUFS
#define LW_H3_BUFS 3             // ... during every stage of the H3 variant (4 spills: 256 registers with 3)
#endif

struct WChunk {
    f32x4 v[8];      // 8 fp32 k-steps (q) of a weight tile, or 4 fp16 k-steps as (hi, lo) pairs
    float bias;      // first chunk of a tile only: bias of output channel n0 + l31 in lane-half 0, zero in lane-half 1
};

template <int B, int E, class F>
__device__ __forceinline__ void static_for(F&& f) {
    if constexpr (B < E) {
        f(std::integral_constant<int, B>{});
        static_for<B + 1, E>(f);
    }
}

enum { ST_FC1 = 0, ST_FC2, ST_FC3, ST_PCN, ST_QKV };
struct ChunkDesc { int stage, tile, chunk, nchunks; };

// F (pdsc_config.value_fold): the folded layer -- fc1 lives in the value projection (V' = W1f Wv, 64 channels), so the tail
// stream is fc2, fc3 (6 chunks) and the head stream pcn, q, k, v' (28 chunks: q|k|v' has 10 output tiles instead of 12)
template <bool T, bool H, bool F = false>
constexpr int num_chunks() { return (T ? (F ? 6 : 10) : 0) + (H ? (F ? 28 : 32) : 0); }

template <bool T, bool F = false>
constexpr ChunkDesc chunk_desc(int i) {
    if (T) {
        if (!F) {
            if (i < 4) return {ST_FC1, i / 2, i % 2, 2};
            i -= 4;
        }
        if (i < 2) return {ST_FC2, i, 0, 1};
        i -= 2;
        if (i < 4) return {ST_FC3, i, 0, 1};
        i -= 4;
    }
    if (i < 8) return {ST_PCN, i / 2, i % 2, 2};
    i -= 8;
    return {ST_QKV, i / 2, i % 2, 2};
}

// ordinal of the output tile inside its stream (tail: fc1 0..1, fc2 2..3, fc3 4..7; head: pcn 0..3, q|k|v 4..15)
// (folded tail: fc2 0..1, fc3 2..5)
template <bool F = false>
constexpr int tile_ordinal(const ChunkDesc d) {
    constexpr int o = F ? 2 : 0;
    return d.stage == ST_FC1 ? d.tile : d.stage == ST_FC2 ? 2 - o + d.tile : d.stage == ST_FC3 ? 4 - o + d.tile : d.stage == ST_PCN ? d.tile : 4 + d.tile;
}
constexpr int LW_TAIL_CHUNKS = 10, LW_HEAD_CHUNKS = 32, LW_TAIL_TILES = 8, LW_HEAD_TILES = 16;
constexpr int LW_FOLD_TAIL_CHUNKS = 6, LW_FOLD_HEAD_CHUNKS = 28, LW_FOLD_TAIL_TILES = 6, LW_FOLD_HEAD_TILES = 14;
constexpr int LW_FOLD_VW = PDSC_CHANNELS / 2;      // channels of V' (and of the folded attention's partials / messages)
template <bool F> constexpr int tail_chunks() { return F ? LW_FOLD_TAIL_CHUNKS : LW_TAIL_CHUNKS; }
template <bool F> constexpr int head_chunks() { return F ? LW_FOLD_HEAD_CHUNKS : LW_HEAD_CHUNKS; }
// folded tail stream: chunks, bias fragments, then b' = W1f bv + b1f (64 fp32) -- the bias of the merged 64-channel message
constexpr int LW_FOLD_BPRIME_BYTES = LW_FOLD_TAIL_CHUNKS * 8192 + LW_FOLD_TAIL_TILES * 256;

__device__ __forceinline__ void load_rows_f32(WChunk& w, const float* __restrict__ p) {
#pragma unroll
    for (int q = 0; q < 8; ++q) w.v[q] = *reinterpret_cast<const f32x4*>(p + 8 * q);
}

constexpr int LW_CHUNK_BYTES = 8192;      // one WChunk for all 64 lanes

// chunk `idx` of a fragment-ordered stream (pdsc_wfrag_build_*): slot s of lane l is the 16 bytes at s*1024 + l*16, i.e.
// every load instruction of the wave reads 1 KiB of consecutive memory (8 cache lines).  The natural [out][in] layout
// below makes the same instruction touch 64 different lines (row stride 256..512 B), which serialises in the L1.
// The bias fragments (256 B per output tile) follow the chunks of the stream.
__device__ __forceinline__ void load_chunk_frag(WChunk& w, const unsigned char* __restrict__ stream, int idx, int nchunks,
                                                int bias_tile /* -1: not the first chunk of a tile */, int lane) {
    const unsigned char* p = stream + (size_t)idx * LW_CHUNK_BYTES + lane * 16;
#pragma unroll
    for (int s = 0; s < 8; ++s) w.v[s] = *reinterpret_cast<const f32x4*>(p + 1024 * s);
    if (bias_tile >= 0) w.bias = *reinterpret_cast<const float*>(stream + (size_t)nchunks * LW_CHUNK_BYTES + bias_tile * 256 + lane * 4);
}

template <bool T, bool X3, bool FRAG, bool F = false>
__device__ __forceinline__ void load_chunk(WChunk& w, const LayerArgs& a, const int i, int lane) {
    const ChunkDesc d = chunk_desc<T, F>(i);
    const int bias_tile = d.chunk == 0 ? tile_ordinal<F>(d) : -1;
    static_assert(FRAG || !F, "the folded layer takes fragment streams");
    if (FRAG) {
        if (T && i < tail_chunks<F>()) load_chunk_frag(w, a.wf_tail, i, tail_chunks<F>(), bias_tile, lane);
        else load_chunk_frag(w, a.wf_head, i - (T ? tail_chunks<F>() : 0), head_chunks<F>(), bias_tile, lane);
        return;
    }
    const int l31 = lane & 31, h = lane >> 5;
    const int n = 32 * d.tile + l31;
    if (d.chunk == 0) {
        const float* b = d.stage == ST_FC1 ? a.b1 : d.stage == ST_FC2 ? a.b2 : d.stage == ST_FC3 ? a.b3 : d.stage == ST_PCN ? a.bp : a.bq;
        const float bv = b[n];
        w.bias = h ? 0.f : bv;
    }
    switch (d.stage) {
        case ST_FC1: load_rows_f32(w, a.w1 + (size_t)n * 128 + 64 * d.chunk + 4 * h); break;
        case ST_FC2: load_rows_f32(w, a.w2 + (size_t)n * 64 + 4 * h); break;
        case ST_FC3: load_rows_f32(w, a.w3 + (size_t)n * 64 + 4 * h); break;
        case ST_PCN: load_rows_f32(w, a.wp + (size_t)n * 128 + 64 * d.chunk + 4 * h); break;
        default:
            if (X3) {
                const sp16* p = a.wq_split + (size_t)n * PDSC_CHANNELS + 64 * d.chunk + 8 * h;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    w.v[2 * k] = *reinterpret_cast<const f32x4*>(p + 16 * k);
                    w.v[2 * k + 1] = *reinterpret_cast<const f32x4*>(p + (size_t)3 * PDSC_CHANNELS * PDSC_CHANNELS + 16 * k);
                }
            } else {
                load_rows_f32(w, a.wq + (size_t)n * 128 + 64 * d.chunk + 4 * h);
            }
    }
}

__device__ __forceinline__ void mma_f32(f32x16& acc, const WChunk& w, const f32x4* x) {
#pragma unroll
    for (int q = 0; q < 8; ++q)
#pragma unroll
        for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(w.v[q][e], x[q][e], acc, 0, 0, 0);
}

// accumulator := bias, on the matrix pipe: one extra k-step whose A operand is the bias fragment (zero in the second k slot) and
// whose B operand is 1 -- no VALU work, and C = 0 is an inline constant
__device__ __forceinline__ f32x16 bias_step(const WChunk& w) {
    const f32x16 zero = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    return __builtin_amdgcn_mfma_f32_32x32x2f32(w.bias, 1.0f, zero, 0, 0, 0);
}

// one weight chunk (4 k-steps as (hi, lo) slot pairs) of the split q|k|v projection: small terms first, one accumulator
__device__ __forceinline__ void mma_x3(f32x16& acc, const WChunk& w, const u32x4* xh, const u32x4* xl) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const sp16x8 wh = __builtin_bit_cast(sp16x8, w.v[2 * i]), wl = __builtin_bit_cast(sp16x8, w.v[2 * i + 1]);
        const sp16x8 bh = __builtin_bit_cast(sp16x8, xh[i]), bl = __builtin_bit_cast(sp16x8, xl[i]);
        acc = PDSC_MFMA_X3(wl, bh, acc, 0, 0, 0);
        acc = PDSC_MFMA_X3(wh, bl, acc, 0, 0, 0);
        acc = PDSC_MFMA_X3(wh, bh, acc, 0, 0, 0);
    }
}

__device__ __forceinline__ unsigned pack2(sp16 a, sp16 b) {
    return (unsigned)__builtin_bit_cast(unsigned short, a) | ((unsigned)__builtin_bit_cast(unsigned short, b) << 16);
}

typedef float f32x2 __attribute__((ext_vector_type(2)));

// two fp32 -> packed hi pair and lo pair of the x3 split (split_layout.h: split_sp16_pair)
__device__ __forceinline__ void split2(float x0, float x1, unsigned& hi, unsigned& lo) { split_sp16_pair(x0, x1, hi, lo); }

// fp32 x4 -> packed hi (2 registers) and lo (2 registers)
__device__ __forceinline__ void split4(const f32x4& v, unsigned (&hi)[2], unsigned (&lo)[2]) {
    split2(v[0], v[1], hi[0], lo[0]);
    split2(v[2], v[3], hi[1], lo[1]);
}

// ---- fp16 hi / scaled-lo split (the H3 arithmetic of the fc1..fc3 / PointCN GEMMs) -----------------------------------
// x = hi + lo' / 2048 with hi = f16(x), lo' = f16((x - hi) * 2048), both round-to-nearest-even.  hi carries 11
// significant bits, lo' the next 11: a product a*b evaluated as  a_hi*b_hi + (a_hi*b_lo' + a_lo'*b_hi) / 2048  on
// v_mfma_f32_32x32x16_f16 (fp32 accumulate, the two cross terms in their own accumulator) is exact to ~2^-21 relative,
// which is what lets the GEMMs that land on the residual stream leave the fp32 MFMA (1/16 of the f16 rate).  The scale keeps
// lo' in the normal range of fp16 whenever hi is (the attention operands' split, split_layout.h, is the same pair WITHOUT the
// scale -- one accumulator for all three terms -- and therefore has an absolute floor of 2^-25 on lo).  Range: |x| < 65504 (fp16); activations and weights of this network are O(1).
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
constexpr float H3_SCALE = 2048.0f, H3_INV = 1.0f / 2048.0f;

__device__ __forceinline__ void split2h(float x0, float x1, unsigned& hi, unsigned& lo) {
    const f16x2 hv = __builtin_convertvector(f32x2{x0, x1}, f16x2);
    hi = __builtin_bit_cast(unsigned, hv);
    const f32x2 hf = __builtin_convertvector(hv, f32x2);
    const f16x2 lv = __builtin_convertvector(f32x2{(x0 - hf[0]) * H3_SCALE, (x1 - hf[1]) * H3_SCALE}, f16x2);
    lo = __builtin_bit_cast(unsigned, lv);
}

__device__ __forceinline__ void split4h(const f32x4& v, unsigned (&hi)[2], unsigned (&lo)[2]) {
    split2h(v[0], v[1], hi[0], lo[0]);
    split2h(v[2], v[3], hi[1], lo[1]);
}

// v_permlane32_swap: lanes 32..63 of `a` trade places with lanes 0..31 of `b`.
// afterwards, per lane: lower half (a, b) = (own a, partner's a);  upper half (a, b) = (partner's b, own b).
__device__ __forceinline__ void half_swap(unsigned& a, unsigned& b) {
    const auto r = __builtin_amdgcn_permlane32_swap(a, b, false, false);
    a = r[0];
    b = r[1];
}

// Lane-half h holds 4 consecutive channels (c0+4h..+3) of a value as packed hi[2] / lo[2].  Returns the 16-byte chunk
// this lane stores: lower half -> the 8 hi values of channels c0..c0+7, upper half -> the 8 lo values.
__device__ __forceinline__ u32x4 chunk_for_store(const unsigned (&hi)[2], const unsigned (&lo)[2]) {
    unsigned a0 = hi[0], b0 = lo[0], a1 = hi[1], b1 = lo[1];
    half_swap(a0, b0);        // lower: (own hi0, partner hi0); upper: (partner lo0, own lo0)
    half_swap(a1, b1);
    // lower half: own = channels 0..3, partner = 4..7 -> (a0, a1, b0, b1); upper: partner = 0..3 (a), own = 4..7 (b)
    return u32x4{a0, a1, b0, b1};
}

// B operand of one 16-wide k-step kk from the fp32 accumulator layout: lane-half h holds `a` = channels 16kk + 4h + e and
// `b` = channels 16kk + 8 + 4h + e of its point; the k-step wants channels 16kk + 8h .. +7 in lane-half h.  F16 selects the
// fp16 hi / scaled-lo split (H3) instead of the unscaled fp16 hi / lo split.
template <bool F16>
__device__ __forceinline__ void make_kstep(const f32x4& a, const f32x4& b, u32x4& oh, u32x4& ol) {
    unsigned ha[2], la[2], hb[2], lb[2];
    if constexpr (F16) { split4h(a, ha, la); split4h(b, hb, lb); }
    else { split4(a, ha, la); split4(b, hb, lb); }
    half_swap(ha[0], hb[0]); half_swap(ha[1], hb[1]);
    half_swap(la[0], lb[0]); half_swap(la[1], lb[1]);
    oh = u32x4{ha[0], ha[1], hb[0], hb[1]};
    ol = u32x4{la[0], la[1], lb[0], lb[1]};
}

// ... with the values noted by the fp16 range sentinel (pdsc_common.h)
template <bool F16>
__device__ __forceinline__ void make_kstep(const f32x4& a_in, const f32x4& b_in, u32x4& oh, u32x4& ol, float& rmax) {
    f32x4 a = a_in, b = b_in;
    range_note(rmax, a);
    range_note(rmax, b);
    make_kstep<F16>(a, b, oh, ol);
}

// one weight chunk (4 k-steps as (hi, lo') slot pairs) in the H3 arithmetic: main accumulator <- hi*hi, cross <- the two
// hi*lo' terms (scaled by 2048; folded in by the tile epilogue)
__device__ __forceinline__ void mma_h3(f32x16& acc, f32x16& cross, const WChunk& w, const u32x4* xh, const u32x4* xl, bool first) {
    const f32x16 zero = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const f16x8 wh = __builtin_bit_cast(f16x8, w.v[2 * i]), wl = __builtin_bit_cast(f16x8, w.v[2 * i + 1]);
        const f16x8 bh = __builtin_bit_cast(f16x8, xh[i]), bl = __builtin_bit_cast(f16x8, xl[i]);
        cross = __builtin_amdgcn_mfma_f32_32x32x16_f16(wl, bh, (first && i == 0) ? zero : cross, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(wh, bh, acc, 0, 0, 0);
        cross = __builtin_amdgcn_mfma_f32_32x32x16_f16(wh, bl, cross, 0, 0, 0);
    }
}

// ---- output staging ---------------------------------------------------------------------------------------------------
// In the accumulator layout a lane owns 16 bytes of 32 different rows, so a direct global store touches 64 cache lines
// and costs the L1 64 cycles (measured: 73 us of a 310 us launch at 32 pairs went into such stores).  Outputs therefore
// pass through a wave-private LDS patch of 32 rows x 144 B (128 B payload + 16 B pad) and leave as contiguous runs:
// lane = (row 8*it + lane/8, 16-byte piece lane%8), four passes.  Wave-private: ordering needs no workgroup barrier.
constexpr int LW_PROW = LW_VLD * 4;        // bytes per patch row

__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// ---- the 32-point tile of a wavefront (layer_coop.hip: of a workgroup) -----------------------------------------------------
// tile `gw` of the launch = tile `tile` of pair b, rows m0 .. m0 + valid - 1.  valid <= 0: nothing to do (past the launch's last
// tile, or, in a ragged batch, past the pair's own rows).  Lane (l31, h) works on row `row`; lanes beyond the pair's last point
// (!live) on a copy of its last row.
struct TileDesc {
    int b, tile, m0, valid;
    bool live;
    size_t row;
};
__device__ __forceinline__ TileDesc tile_desc(const LayerArgs& a, int gw, int l31) {
    const int tpp = ceil_div_dev(a.N, 32);                          // tiles per pair
    TileDesc t{};
    if (gw >= a.bs * tpp) return t;
    t.b = gw / tpp;
    t.tile = gw - t.b * tpp;
    t.m0 = t.b * a.N + t.tile * 32;
    t.valid = min(32, (a.nvalid ? a.nvalid[t.b] : a.N) - t.tile * 32);
    t.live = l31 < t.valid;
    t.row = (size_t)t.m0 + min(l31, t.valid - 1);
    return t;
}

// ---- writers of the attention's operand streams (split_layout.h) and of featB rows, one step each ------------------------------
// v = piece g of an output tile: channels n0 + 8g + 4h + e of point l31 in lane (l31, h).  layer_h3_kernel issues the steps one at
// a time between MFMA groups, the other kernels in loops.  Which rows a line store covers (predicated, or clamped to copies of the
// last row) is the caller's: the stores take the row.

// piece g of a featB tile into the patch: row l31 = the tile's 32 channels as fp32 (128 B)
__device__ __forceinline__ void patch_put_featB(unsigned char* patch, int lane, int g, const f32x4& v) {
    *reinterpret_cast<f32x4*>(patch + (lane & 31) * LW_PROW + 32 * g + 16 * (lane >> 5)) = v;
}
// pass `it` of 4 over the patch: lane = (row 8 it + lane / 8, 16-byte piece lane % 8), i.e. 8 rows x 128 B per instruction
__device__ __forceinline__ int patch_line_row(int lane, int it) { return 8 * it + (lane >> 3); }
__device__ __forceinline__ u32x4 patch_line(const unsigned char* patch, int lane, int it) {
    return *reinterpret_cast<const u32x4*>(patch + patch_line_row(lane, it) * LW_PROW + 16 * (lane & 7));
}
// ... and its store as 128 B of row `m` of featB (channels n0 ..)
__device__ __forceinline__ float* featB_line(float* featB, size_t m, int n0, int lane) { return featB + m * PDSC_CHANNELS + n0 + 4 * (lane & 7); }

// keys beyond the pair's end are zero in the K and V^T images
__device__ __forceinline__ f32x4 zero_unless(bool live, const f32x4& v) {
    f32x4 z;
#pragma unroll
    for (int e = 0; e < 4; ++e) z[e] = live ? v[e] : 0.f;
    return z;
}
// K image, chunk-major: after the half swap lane (key l31, half h) holds chunk `chunk` of its key for the hi (h = 0) / lo (h = 1)
// plane -- the 32 lanes of a half store 512 consecutive, aligned bytes
__device__ __forceinline__ u32x4 k_chunk(const f32x4& v, bool live) {
    unsigned hi[2], lo[2];
    split4(zero_unless(live, v), hi, lo);
    return chunk_for_store(hi, lo);
}
__device__ __forceinline__ void k_chunk_store(unsigned char* img, int lane, int chunk, const u32x4& ck) {
    *reinterpret_cast<u32x4*>(img + ((lane >> 5) ? SPL_KL : SPL_KH) + spl_k_offset(lane & 31, chunk)) = ck;
}

// V^T image: 32 keys x 32 channels are transposed through the patch (as floats, LW_VLD per key row)
__device__ __forceinline__ void vt_put(float* Vs, int lane, int g, const f32x4& z) {
    *reinterpret_cast<f32x4*>(Vs + (lane & 31) * LW_VLD + 8 * g + 4 * (lane >> 5)) = z;
}
// pass `it` of 2: lane = (channel 16 it + lane / 4 of the tile, key chunk jh = lane % 4) gathers its chunk's 8 keys ...
__device__ __forceinline__ int vt_channel(int lane, int it) { return 16 * it + (lane >> 2); }
__device__ __forceinline__ void vt_gather(const float* Vs, int lane, int it, float (&vt)[8]) {
#pragma unroll
    for (int e = 0; e < 8; ++e) vt[e] = Vs[spl_v_key(lane & 3, e) * LW_VLD + vt_channel(lane, it)];
}
// ... splits them into the 16 bytes of the hi and of the lo plane ...
__device__ __forceinline__ void vt_split(const float (&vt)[8], u32x4& ch, u32x4& cl) {
    unsigned hi[4], lo[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) split2(vt[2 * e], vt[2 * e + 1], hi[e], lo[e]);
    ch = u32x4{hi[0], hi[1], hi[2], hi[3]};
    cl = u32x4{lo[0], lo[1], lo[2], lo[3]};
}
// ... and stores them at channel n0 + vt_channel of the image (VW channels per plane): 256-byte runs of 16 channels
template <int VW>
__device__ __forceinline__ int vt_offset(int lane, int it, int n0) { return spl_v_offset_w<VW>(n0 + vt_channel(lane, it), lane & 3); }
template <int VW>
__device__ __forceinline__ void vt_store(unsigned char* img, int off, const u32x4& ch, const u32x4& cl) {
    *reinterpret_cast<u32x4*>(img + SPL_VH + off) = ch;
    *reinterpret_cast<u32x4*>(img + spl_v_lo<VW>() + off) = cl;
}

}  // namespace pdsc
