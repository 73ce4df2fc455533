// a-2 fused, wavefront-resident: the whole point-wise chain between two attention calls for one 32-point tile runs in
// ONE wavefront, with every activation in registers.
//   tail of layer i   : feat  = featB + fc3( relu(fc2'( relu(fc1'(msg)) )) )         (reference models/PointDSC.py:43-45)
//   head of layer i+1 : featB = relu(pcn'(feat)) ; (q|k|v) = Wqkv featB + b            (models/PointDSC.py:75, :36-38)
// Why one wave per tile: with D = W_tile (A operand, rows = output channels) x X^T (B operand, columns = points) on
// v_mfma_f32_32x32x2_f32 the accumulator register r = 4g+e of lane (point p, half h) holds output channel n0+8g+4h+e, and
// the B operand of the NEXT GEMM wants, in k-step 4q+e, channel 8q+4h+e of point p in the same lane: the accumulator of
// output tile n0 IS the next stage's operand for k-steps q = n0/8 .. n0/8+3.  So a wave that computes all output tiles
// of a stage feeds the next stage without LDS, without barriers, and waves never wait for each other: a CU holds 8
// independent chains (2 per SIMD) that hide each other's weight-fetch latency.  (layer.hip, the previous design, spreads
// the tiles of a stage over 4 waves and pays 13 workgroup barriers per tile; it measured 3 x the MFMA time.)
// Weights stream from L2 straight into registers in 32-register chunks (8 k-steps), one chunk ahead of the MFMAs.
// The q|k|v projection runs in split precision (hi*hi + hi*lo + lo*hi on v_mfma_f32_32x32x16_f16) when wq_split is
// given; its 16-wide k-step takes channels 16kk+8h..+7 from lane-half h, i.e. two lanes' worth of the fp32 layout, which
// one v_permlane32_swap per register pair rearranges.  The same swap turns the (4 channels per lane-half) accumulator
// layout into the 16-byte (8 channels) chunks of the Q rows / K image (split_layout.h); only V^T needs a transpose
// through a wave-private 4.5 KiB LDS patch.
// Bound: MFMA, 46k matrix-pipe cycles per tile (fp32 stages 36.9k + split q|k|v 9.2k).
#include <stdlib.h>
#include <type_traits>
#include "pdsc_common.h"
#include "split_layout.h"
#include "merge_partials.h"
#include "layer_args.h"

#include "layer_wave.h"

namespace pdsc {

// diagnostics (pdsc_layer_trace): 64 shader-clock stamps per wave: 0 start, 1 input in registers, 2+i chunk i done, 63 end
#define LW_STAMP(k) \
    if (TRACE && lane == 0) a.trace[(size_t)gw * 64 + (k)] = __builtin_readcyclecounter();

// HX: fc1..fc3 and PointCN in the fp16 hi / scaled-lo arithmetic (H3, layer_wave.h) on fragment streams built with
// format PDSC_LAYER_GEMM_H3 -- 504 f16 MFMAs (16.1 k matrix-pipe cycles) per tile instead of 600 fp32 + 288 f16 (46 k).
template <bool T, bool H, bool X3, bool FRAG, bool TRACE = false, bool HX = false>
__global__ __launch_bounds__(64 * LW_WAVES, 2) void layer_wave_kernel(LayerArgs a) {
    static_assert(!HX || (FRAG && (X3 || !H)), "H3 GEMMs read fragment streams");
    __shared__ __attribute__((aligned(16))) float Vs_all[LW_WAVES][32 * LW_VLD];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int l31 = lane & 31, h = lane >> 5;
    const int gw = blockIdx.x * LW_WAVES + wave;                    // one wave = one tile
    const TileDesc td = tile_desc(a, gw, l31);
    if (td.valid <= 0) return;                                       // (no workgroup barriers anywhere below)
    const int m0 = td.m0, valid = td.valid;
    const bool live = td.live;
    const size_t row = td.row;
    float* Vs = Vs_all[wave];
    unsigned char* patch = reinterpret_cast<unsigned char*>(Vs);     // the same 32 x 144 B patch, as bytes

    LW_STAMP(0)
    constexpr int NCH = num_chunks<T, H>();
    // weight ring: the fp32 chunks (2048 matrix-pipe cycles each) are fetched one chunk ahead in two buffers; the split
    // q|k|v chunks (384 cycles each, far less than an L2 round trip) NQB-1 chunks ahead in NQB buffers
    // (HX: every chunk is 12 short MFMAs, so the deep ring serves all of them)
    constexpr int Q0 = HX ? 0 : (H && X3) ? (T ? 10 : 0) + 8 : NCH;  // first chunk on the deep ring
    constexpr int NQB = HX ? LW_H3_BUFS : (H && X3) ? (FRAG ? LW_QKV_BUFS : LW_QKV_BUFS - 1) : 2;     // (natural layout: more address registers)
    WChunk w[NQB];
    auto buf_of = [](int i) constexpr { return i < Q0 ? (i & 1) : (i - Q0) % NQB; };
    load_chunk<T, X3, FRAG>(w[0], a, 0, lane);

    f32x4 x0[16], x1[8], x2[8], y3[16], x4[16];
    u32x4 xh[8], xl[8];                                              // X3: B operands of q|k|v
    u32x4 a0h[8], a0l[8], a1h[4], a1l[4], a2h[4], a2l[4], ayh[8], ayl[8];     // HX: B operands of fc1 / fc2 / fc3 / PointCN
    if (T) {
        if (a.msg) {
#pragma unroll
            for (int q = 0; q < 16; ++q) x0[q] = *reinterpret_cast<const f32x4*>(a.msg + row * PDSC_CHANNELS + 8 * q + 4 * h);
            if constexpr (HX) {
#pragma unroll
                for (int kk = 0; kk < 8; ++kk) make_kstep<true>(x0[2 * kk], x0[2 * kk + 1], a0h[kk], a0l[kk]);
            }
        } else {
            with_split_count<MERGE_MAX_SPLIT>(a.nsplit, [&](auto ns_tag) {
                constexpr int NS = decltype(ns_tag)::value;
                constexpr int GQ = NS <= 2 ? 16 : 8;                 // pieces per batch of loads (up to 128 registers in flight)
                const size_t slot0 = (size_t)td.b * NS * a.Npad + (row - (size_t)td.b * a.N);
                const MergeWeights<NS> mw = merge_row_weights<NS>(a.part_ml, slot0, (size_t)a.Npad);
                // (rows only, own addresses: <1,0,0,1,0,1> has 221 registers with them, 222 through a shared address helper)
#pragma unroll
                for (int q0 = 0; q0 < 16; q0 += GQ) {
                    f32x4 pv[GQ][NS];
#pragma unroll
                    for (int q = 0; q < GQ; ++q)
#pragma unroll
                        for (int sp = 0; sp < NS; ++sp) pv[q][sp] = *reinterpret_cast<const f32x4*>(a.part_o + (slot0 + (size_t)sp * a.Npad) * PDSC_CHANNELS + 8 * (q0 + q) + 4 * h);
#pragma unroll
                    for (int q = 0; q < GQ; ++q) {
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            x0[q0 + q][e] = merge_apply<NS>(pv[q], mw, e);
                            asm volatile("" : "+v"(x0[q0 + q][e]));     // materialise here (else the compiler sinks the arithmetic
                        }                                               // to the first MFMA and keeps every batch of loads live)
                    }
                    if constexpr (HX) {
#pragma unroll
                        for (int kk = q0 / 2; kk < (q0 + GQ) / 2; ++kk) make_kstep<true>(x0[2 * kk], x0[2 * kk + 1], a0h[kk], a0l[kk]);
                    }
                    __builtin_amdgcn_sched_barrier(0);               // keep the next batch's loads behind this batch's use
                }
            });
        }
    } else {
#pragma unroll
        for (int q = 0; q < 16; ++q) y3[q] = *reinterpret_cast<const f32x4*>(a.feat_in + row * PDSC_CHANNELS + 8 * q + 4 * h);
        if constexpr (HX) {
#pragma unroll
            for (int kk = 0; kk < 8; ++kk) make_kstep<true>(y3[2 * kk], y3[2 * kk + 1], ayh[kk], ayl[kk]);
        }
    }
    LW_STAMP(1)

    unsigned char* img = (H && a.kv) ? a.kv + (size_t)gw * SPL_TILE_STRIDE : nullptr;
    f32x16 acc, cross;
    // fp16 range sentinel (pdsc_common.h) of the fp32-GEMM forms: what they convert to fp16 pairs is the PointCN output (operand of the
    // split q|k|v projection) and q, k, v (the attention's streams).  The generic H3 form (HX) carries none: no forward runs it
    constexpr bool RANGE = H && X3 && !HX;
    float rmax = 0.f;

    static_for<0, NCH>([&](auto ic) {
        constexpr int i = decltype(ic)::value;
        constexpr ChunkDesc d = chunk_desc<T>(i);
        constexpr int n0 = 32 * d.tile;
        if constexpr (i < Q0) {
            if constexpr (i + 1 < NCH) load_chunk<T, X3, FRAG>(w[buf_of(i + 1)], a, i + 1, lane);
        } else if constexpr (i == Q0) {
            static_for<1, NQB>([&](auto jc) {
                constexpr int j = Q0 + decltype(jc)::value;
                if constexpr (j < NCH) load_chunk<T, X3, FRAG>(w[buf_of(j)], a, j, lane);
            });
        } else if constexpr (i + NQB - 1 < NCH) {
            load_chunk<T, X3, FRAG>(w[buf_of(i + NQB - 1)], a, i + NQB - 1, lane);
        }
        if constexpr (T && d.stage == ST_FC2 && d.tile == 0) {
            // residual rows for fc3's epilogue, two chunks early (x0 is dead, its registers are free): they come from HBM
#pragma unroll
            for (int q = 0; q < 16; ++q) y3[q] = *reinterpret_cast<const f32x4*>(a.res + row * PDSC_CHANNELS + 8 * q + 4 * h);
        }
        const WChunk& wc = w[buf_of(i)];
        if constexpr (d.chunk == 0) {
            acc = bias_step(wc);
        }
        if constexpr (HX && d.stage == ST_FC1) mma_h3(acc, cross, wc, a0h + 4 * d.chunk, a0l + 4 * d.chunk, d.chunk == 0);
        else if constexpr (HX && d.stage == ST_FC2) mma_h3(acc, cross, wc, a1h, a1l, true);
        else if constexpr (HX && d.stage == ST_FC3) mma_h3(acc, cross, wc, a2h, a2l, true);
        else if constexpr (HX && d.stage == ST_PCN) mma_h3(acc, cross, wc, ayh + 4 * d.chunk, ayl + 4 * d.chunk, d.chunk == 0);
        else if constexpr (d.stage == ST_FC1) mma_f32(acc, wc, x0 + 8 * d.chunk);
        else if constexpr (d.stage == ST_FC2) mma_f32(acc, wc, x1);
        else if constexpr (d.stage == ST_FC3) mma_f32(acc, wc, x2);
        else if constexpr (d.stage == ST_PCN) mma_f32(acc, wc, y3 + 8 * d.chunk);
        else if constexpr (X3) mma_x3(acc, wc, xh + 4 * d.chunk, xl + 4 * d.chunk);
        else mma_f32(acc, wc, x4 + 8 * d.chunk);

        if constexpr (d.chunk == d.nchunks - 1) {
            // ---- epilogue of output tile n0: lane (point l31, half h) holds channels n0 + 8g + 4h + e ----
            f32x4 v[4];
#pragma unroll
            for (int g = 0; g < 4; ++g)
#pragma unroll
                for (int e = 0; e < 4; ++e) v[g][e] = (HX && d.stage != ST_QKV) ? fmaf(cross[4 * g + e], H3_INV, acc[4 * g + e]) : acc[4 * g + e];
            if constexpr (HX && (d.stage == ST_FC1 || d.stage == ST_FC2)) {
                // relu, then straight into the next GEMM's k-steps 2*tile, 2*tile + 1 (this tile's 32 channels)
#pragma unroll
                for (int g = 0; g < 4; ++g)
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[g][e] = fmaxf(v[g][e], 0.f);
#pragma unroll
                for (int j = 0; j < 2; ++j)
                    make_kstep<true>(v[2 * j], v[2 * j + 1], (d.stage == ST_FC1 ? a1h : a2h)[2 * d.tile + j], (d.stage == ST_FC1 ? a1l : a2l)[2 * d.tile + j]);
            } else if constexpr (d.stage == ST_FC1 || d.stage == ST_FC2) {
#pragma unroll
                for (int g = 0; g < 4; ++g)
#pragma unroll
                    for (int e = 0; e < 4; ++e) (d.stage == ST_FC1 ? x1 : x2)[4 * d.tile + g][e] = fmaxf(v[g][e], 0.f);
            } else if constexpr (d.stage == ST_FC3) {
#pragma unroll
                for (int g = 0; g < 4; ++g) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) y3[4 * d.tile + g][e] = y3[4 * d.tile + g][e] + v[g][e];
                    if (a.feat_out && live)
                        *reinterpret_cast<f32x4*>(a.feat_out + row * PDSC_CHANNELS + n0 + 8 * g + 4 * h) = y3[4 * d.tile + g];
                }
                if constexpr (HX && H) {
#pragma unroll
                    for (int j = 0; j < 2; ++j)
                        make_kstep<true>(y3[4 * d.tile + 2 * j], y3[4 * d.tile + 2 * j + 1], ayh[2 * d.tile + j], ayl[2 * d.tile + j]);
                }
            } else if constexpr (d.stage == ST_PCN) {
#pragma unroll
                for (int g = 0; g < 4; ++g) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) x4[4 * d.tile + g][e] = fmaxf(v[g][e], 0.f);
                    patch_put_featB(patch, lane, g, x4[4 * d.tile + g]);
                }
                wave_lds_sync();
#pragma unroll
                for (int it = 0; it < 4; ++it) {          // 8 points x 128 B (one full line each) per store instruction
                    const int pt = patch_line_row(lane, it);
                    const u32x4 val = patch_line(patch, lane, it);
                    if (pt < valid) *reinterpret_cast<u32x4*>(featB_line(a.featB_out, (size_t)m0 + pt, n0, lane)) = val;
                }
                wave_lds_sync();
                if constexpr (X3 && d.tile == 3) {
                    // featB -> fp16 hi / lo operands of the 16-wide k-steps: step kk, lane-half h <- channels 16kk+8h..+7
#pragma unroll
                    for (int kk = 0; kk < 8; ++kk) {
                        if constexpr (RANGE) make_kstep<false>(x4[2 * kk], x4[2 * kk + 1], xh[kk], xl[kk], rmax);
                        else make_kstep<false>(x4[2 * kk], x4[2 * kk + 1], xh[kk], xl[kk]);
                    }
                }
            } else {
                // q | k | v, output tile d.tile of 12: tiles 0..3 = q, 4..7 = k, 8..11 = v
                // (the three writers below are this kernel's own text: <0,1,0,0,0,0> has 198 registers with it and 200 through the
                //  step helpers of layer_wave.h, <*,1,1,1,0,0> 233 and 238; its K image goes through the patch and its row stores are
                //  predicated, which the helpers' users do not do)
                if (a.qkv_out && live) {
#pragma unroll
                    for (int g = 0; g < 4; ++g)
                        *reinterpret_cast<f32x4*>(a.qkv_out + row * (3 * PDSC_CHANNELS) + n0 + 8 * g + 4 * h) = v[g];
                }
                if (a.qs) {
                    if constexpr (d.tile < 4) {
                        // patch row = (hi 64 B | lo 64 B) of this tile's 32 channels: lower lane-half holds hi chunks, upper lo
#pragma unroll
                        for (int g = 0; g < 4; ++g) {
                            unsigned hi[2], lo[2];
                            if constexpr (RANGE) range_note(rmax, v[g]);
                            split4(v[g], hi, lo);
                            *reinterpret_cast<u32x4*>(patch + l31 * LW_PROW + 64 * h + 16 * g) = chunk_for_store(hi, lo);
                        }
                        wave_lds_sync();
#pragma unroll
                        for (int it = 0; it < 4; ++it) {
                            const int pt = 8 * it + (lane >> 3), piece = lane & 7;
                            const u32x4 val = *reinterpret_cast<const u32x4*>(patch + pt * LW_PROW + 16 * piece);
                            sp16* dst = a.qs + ((size_t)m0 + pt) * SPL_Q_LD + (piece >> 2) * PDSC_CHANNELS + n0 + 8 * (piece & 3);
                            if (pt < valid) *reinterpret_cast<u32x4*>(dst) = val;
                        }
                        wave_lds_sync();
                    } else if constexpr (d.tile < 8) {
#pragma unroll
                        for (int g = 0; g < 4; ++g) {
                            f32x4 z = v[g];
                            if (valid < 32) {                                                    // wave-uniform: last tile of a pair
#pragma unroll
                                for (int e = 0; e < 4; ++e) z[e] = live ? z[e] : 0.f;            // keys beyond N are zero
                            }
                            unsigned hi[2], lo[2];
                            if constexpr (RANGE) range_note(rmax, z);
                            split4(z, hi, lo);
                            *reinterpret_cast<u32x4*>(patch + l31 * LW_PROW + 64 * h + 16 * g) = chunk_for_store(hi, lo);
                        }
                        wave_lds_sync();
#pragma unroll
                        for (int it = 0; it < 4; ++it) {          // 64-byte runs: chunks 4t..4t+3 of a key, hi plane then lo plane
                            const int key = 8 * it + (lane >> 3), piece = lane & 7;
                            const u32x4 val = *reinterpret_cast<const u32x4*>(patch + key * LW_PROW + 16 * piece);
                            *reinterpret_cast<u32x4*>(img + ((piece >> 2) ? SPL_KL : SPL_KH) + spl_k_offset(key, 4 * (d.tile - 4) + (piece & 3))) = val;
                        }
                        wave_lds_sync();
                    } else {
                        // V^T image: transpose 32 keys x 32 channels through the wave-private LDS patch
#pragma unroll
                        for (int g = 0; g < 4; ++g) {
                            f32x4 z = v[g];
                            if (valid < 32) {
#pragma unroll
                                for (int e = 0; e < 4; ++e) z[e] = live ? z[e] : 0.f;
                            }
                            if constexpr (RANGE) range_note(rmax, z);      // (noted before the transpose: split2 below sees the same values)
                            *reinterpret_cast<f32x4*>(Vs + l31 * LW_VLD + 8 * g + 4 * h) = z;
                        }
                        wave_lds_sync();
#pragma unroll
                        for (int it = 0; it < 2; ++it) {          // lane = (channel 16*it + lane/4, key chunk lane%4): 64-byte runs
                            const int cl = 16 * it + (lane >> 2), jh = lane & 3;
                            unsigned chi[4], clo[4];
#pragma unroll
                            for (int e = 0; e < 8; e += 2)
                                split2(Vs[spl_v_key(jh, e) * LW_VLD + cl], Vs[spl_v_key(jh, e + 1) * LW_VLD + cl], chi[e / 2], clo[e / 2]);
                            const u32x4 ch = {chi[0], chi[1], chi[2], chi[3]}, cw = {clo[0], clo[1], clo[2], clo[3]};
                            const int off = spl_v_offset(32 * (d.tile - 8) + cl, jh);
                            *reinterpret_cast<u32x4*>(img + SPL_VH + off) = ch;
                            *reinterpret_cast<u32x4*>(img + SPL_VL + off) = cw;
                        }
                        wave_lds_sync();
                    }
                }
            }
        }
        LW_STAMP(2 + i)
        __builtin_amdgcn_sched_barrier(0);      // chunks are the unit of the software pipeline: no code motion across them
    });

    if constexpr (RANGE) range_report(a.range_flag, td.b, rmax);
    LW_STAMP(63)
}

// ---- fragment-ordered weight streams -------------------------------------------------------------------------------
// element (chunk c, slot s, lane l = (l31, h), e) of a stream <- the weight the natural-layout load_chunk puts there
// H3 slot (layer_wave.h): 8 consecutive input channels of one weight row as fp16 hi (part 0) or scaled lo' (part 1)
__device__ __forceinline__ u32x4 wfrag_h3_slot(const float* __restrict__ src, int part) {
    unsigned w[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        unsigned hi, lo;
        split2h(src[2 * e], src[2 * e + 1], hi, lo);
        w[e] = part ? lo : hi;
    }
    return u32x4{w[0], w[1], w[2], w[3]};
}

// F (folded layer, layer_wave.h): fc2, fc3 only, then b' (`bprime`, 64 fp32) behind the bias fragments; w1 / b1 unused
template <bool F = false>
__global__ __launch_bounds__(256) void wfrag_tail_kernel(const float* __restrict__ w1, const float* __restrict__ b1,
                                                         const float* __restrict__ w2, const float* __restrict__ b2,
                                                         const float* __restrict__ w3, const float* __restrict__ b3,
                                                         const float* __restrict__ bprime, float* __restrict__ out, int fmt) {
    constexpr int NC = tail_chunks<F>(), NT = F ? LW_FOLD_TAIL_TILES : LW_TAIL_TILES, TO = F ? 2 : 0;
    const int idx = blockIdx.x * 256 + threadIdx.x;                  // one float4 = (chunk, slot, lane)
    if (idx < NT * 64) {                                             // bias fragments behind the chunks
        const int t = idx >> 6, lane = idx & 63;
        const float* b = t < 2 - TO ? b1 + 32 * t : t < 4 - TO ? b2 + 32 * (t - 2 + TO) : b3 + 32 * (t - 4 + TO);
        out[(size_t)NC * LW_CHUNK_BYTES / 4 + idx] = lane < 32 ? b[lane] : 0.f;
    }
    if (F && idx < LW_FOLD_VW) out[LW_FOLD_BPRIME_BYTES / 4 + idx] = bprime[idx];
    if (idx >= NC * 8 * 64) return;
    const int c = idx >> 9, s = (idx >> 6) & 7, lane = idx & 63, l31 = lane & 31, h = lane >> 5;
    const ChunkDesc d = chunk_desc<true, F>(c);
    const int n = 32 * d.tile + l31;
    const float* src = d.stage == ST_FC1 ? w1 + (size_t)n * 128 + 64 * d.chunk : d.stage == ST_FC2 ? w2 + (size_t)n * 64 : w3 + (size_t)n * 64;
    if (fmt == PDSC_LAYER_GEMM_H3)      // slot 2k = hi, 2k+1 = lo' of the chunk's k-step k: channels 16k + 8h .. +7
        *reinterpret_cast<u32x4*>(out + (size_t)idx * 4) = wfrag_h3_slot(src + 16 * (s >> 1) + 8 * h, s & 1);
    else
        *reinterpret_cast<f32x4*>(out + (size_t)idx * 4) = *reinterpret_cast<const f32x4*>(src + 8 * s + 4 * h);
}

// F (folded layer): q | k | v' with the v' rows (output tiles 8, 9) from `wfold` = W1f Wv [64][128] and no bias
template <bool F = false>
__global__ __launch_bounds__(256) void wfrag_head_kernel(const float* __restrict__ wp, const float* __restrict__ bp,
                                                         const float* __restrict__ wq, const float* __restrict__ bq,
                                                         const float* __restrict__ wfold, unsigned char* __restrict__ out, int fmt) {
    constexpr int NC = head_chunks<F>(), NT = F ? LW_FOLD_HEAD_TILES : LW_HEAD_TILES;
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx < NT * 64) {
        const int t = idx >> 6, lane = idx & 63;
        const float* b = t < 4 ? bp + 32 * t : bq + 32 * (t - 4);
        reinterpret_cast<float*>(out + (size_t)NC * LW_CHUNK_BYTES)[idx] = lane < 32 && !(F && t >= 12) ? b[lane] : 0.f;
    }
    if (idx >= NC * 8 * 64) return;
    const int c = idx >> 9, s = (idx >> 6) & 7, lane = idx & 63, l31 = lane & 31, h = lane >> 5;
    const ChunkDesc d = chunk_desc<false, F>(c);
    const int n = 32 * d.tile + l31;
    if (F && d.stage == ST_QKV && n >= 2 * PDSC_CHANNELS) wq = wfold - (size_t)2 * PDSC_CHANNELS * 128;     // row n of q|k|v' = row n - 256 of wfold
    if (d.stage == ST_PCN && fmt == PDSC_LAYER_GEMM_H3) {
        *reinterpret_cast<u32x4*>(out + (size_t)idx * 16) = wfrag_h3_slot(wp + (size_t)n * 128 + 64 * d.chunk + 16 * (s >> 1) + 8 * h, s & 1);
    } else if (d.stage == ST_PCN) {
        *reinterpret_cast<f32x4*>(out + (size_t)idx * 16) = *reinterpret_cast<const f32x4*>(wp + (size_t)n * 128 + 64 * d.chunk + 8 * s + 4 * h);
    } else {                                                         // slot 2k = hi, 2k+1 = lo of fp16 k-step 4*chunk + k
        const float* src = wq + (size_t)n * 128 + 64 * d.chunk + 16 * (s >> 1) + 8 * h;
        sp16 v[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            sp16 hi, lo;
            split_sp16(src[e], hi, lo);
            v[e] = (s & 1) ? lo : hi;
        }
        *reinterpret_cast<u32x4*>(out + (size_t)idx * 16) = u32x4{pack2(v[0], v[1]), pack2(v[2], v[3]), pack2(v[4], v[5]), pack2(v[6], v[7])};
    }
}

int launch_layer_wave(const LayerArgs& a, bool tail, bool head, hipStream_t st) {
    const int waves = a.bs * ceil_div(a.N, 32);
    const dim3 grid(ceil_div(waves, LW_WAVES)), block(64 * LW_WAVES);
    const bool frag = (!tail || a.wf_tail) && (!head || a.wf_head);
    const bool x3 = head && (a.wq_split || frag);
    const bool h3 = frag && a.gemm_format == PDSC_LAYER_GEMM_H3;
#ifndef PDSC_EXPERIMENTS
    // r06 prune: the product library ships the forms its own forward and its stage-level parity tests reach -- the
    // exact-fp32 path's rows + natural weights, the fp32-GEMM fragment streams behind a split-precision attention (layer_gemm = "f32")
    // and the generic H3 variant (the stage tests compare layer_h3.hip / layer_coop.hip against it, and it serves the output sets those
    // two do not).  The natural-layout split-weight form and the shader-clock trace are compiled in experiments builds only
    // (python -m pointdsc_amd.build --experiments).
    if (a.trace || (x3 && !frag)) {
        set_error("pdsc_layer_run: this form of the wavefront-per-tile kernel (%s) exists in experiments builds of the library only",
                  a.trace ? "shader-clock trace" : "split q|k|v weights in natural layout");
        return PDSC_ERR_ARG;
    }
#endif
    if (tail && head) {
        profile_mark_begin(PDSC_PROF_LAYER, st);
#ifdef PDSC_EXPERIMENTS
        if (h3 && a.trace) hipLaunchKernelGGL((layer_wave_kernel<true, true, true, true, true, true>), grid, block, 0, st, a);
        else if (frag && !h3 && a.trace) hipLaunchKernelGGL((layer_wave_kernel<true, true, true, true, true>), grid, block, 0, st, a);
        else if (x3 && !frag) hipLaunchKernelGGL((layer_wave_kernel<true, true, true, false>), grid, block, 0, st, a);
        else
#endif
        if (h3) hipLaunchKernelGGL((layer_wave_kernel<true, true, true, true, false, true>), grid, block, 0, st, a);
        else if (frag) hipLaunchKernelGGL((layer_wave_kernel<true, true, true, true>), grid, block, 0, st, a);
        else hipLaunchKernelGGL((layer_wave_kernel<true, true, false, false>), grid, block, 0, st, a);
        profile_mark_end(PDSC_PROF_LAYER, st);
    } else if (tail) {
        if (h3) hipLaunchKernelGGL((layer_wave_kernel<true, false, false, true, false, true>), grid, block, 0, st, a);
        else if (frag) hipLaunchKernelGGL((layer_wave_kernel<true, false, false, true>), grid, block, 0, st, a);
        else hipLaunchKernelGGL((layer_wave_kernel<true, false, false, false>), grid, block, 0, st, a);
    } else {
#ifdef PDSC_EXPERIMENTS
        if (x3 && !frag && !h3) hipLaunchKernelGGL((layer_wave_kernel<false, true, true, false>), grid, block, 0, st, a);
        else
#endif
        if (h3) hipLaunchKernelGGL((layer_wave_kernel<false, true, true, true, false, true>), grid, block, 0, st, a);
        else if (frag) hipLaunchKernelGGL((layer_wave_kernel<false, true, true, true>), grid, block, 0, st, a);
        else hipLaunchKernelGGL((layer_wave_kernel<false, true, false, false>), grid, block, 0, st, a);
    }
    return check_launch("pdsc_layer_run(wave)");
}

}  // namespace pdsc

using namespace pdsc;

extern "C" size_t pdsc_wfrag_tail_bytes(void) { return (size_t)LW_TAIL_CHUNKS * LW_CHUNK_BYTES + LW_TAIL_TILES * 256; }
extern "C" size_t pdsc_wfrag_head_bytes(void) { return (size_t)LW_HEAD_CHUNKS * LW_CHUNK_BYTES + LW_HEAD_TILES * 256; }
extern "C" size_t pdsc_wfrag_fold_tail_bytes(void) { return (size_t)LW_FOLD_BPRIME_BYTES + LW_FOLD_VW * sizeof(float); }
extern "C" size_t pdsc_wfrag_fold_head_bytes(void) { return (size_t)LW_FOLD_HEAD_CHUNKS * LW_CHUNK_BYTES + LW_FOLD_HEAD_TILES * 256; }

// ---- the folded layer's weights (pdsc_config.value_fold) -------------------------------------------------------------------
// wfold = W1f Wv [64][128] accumulated in fp64 from the packed fp32 matrices and rounded once; then b' = W1f bv + b1f (64), the
// same way.  One thread per output element.
__global__ __launch_bounds__(256) void value_fold_kernel(const float* __restrict__ w1, const float* __restrict__ b1,
                                                         const float* __restrict__ wv, const float* __restrict__ bv,
                                                         float* __restrict__ wfold) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    constexpr int C = PDSC_CHANNELS, H = PDSC_CHANNELS / 2;
    if (idx < H * C) {
        const int o = idx / C, c = idx % C;
        double acc = 0.0;
        for (int m = 0; m < C; ++m) acc = fma((double)w1[o * C + m], (double)wv[m * C + c], acc);
        wfold[idx] = (float)acc;
    } else if (idx < H * C + H) {
        const int o = idx - H * C;
        double acc = (double)b1[o];
        for (int m = 0; m < C; ++m) acc = fma((double)w1[o * C + m], (double)bv[m], acc);
        wfold[idx] = (float)acc;
    }
}

int pdsc::build_value_fold(const float* w1, const float* b1, const float* wqkv, const float* bqkv, const float* w2, const float* b2,
                           const float* w3, const float* b3, const float* wp, const float* bp, float* wfold, void* tail_out,
                           void* head_out, hipStream_t st) {
    constexpr int C = PDSC_CHANNELS, H = PDSC_CHANNELS / 2;
    hipLaunchKernelGGL(value_fold_kernel, dim3((H * C + H + 255) / 256), dim3(256), 0, st, w1, b1, wqkv + (size_t)2 * C * C, bqkv + 2 * C, wfold);
    hipLaunchKernelGGL(wfrag_tail_kernel<true>, dim3(LW_FOLD_TAIL_CHUNKS * 8 * 64 / 256), dim3(256), 0, st, w1, b1, w2, b2, w3, b3,
                       wfold + H * C, (float*)tail_out, (int)PDSC_LAYER_GEMM_H3);
    hipLaunchKernelGGL(wfrag_head_kernel<true>, dim3(LW_FOLD_HEAD_CHUNKS * 8 * 64 / 256), dim3(256), 0, st, wp, bp, wqkv, bqkv, wfold,
                       (unsigned char*)head_out, (int)PDSC_LAYER_GEMM_H3);
    return check_launch("pdsc_wsplit_build(value fold)");
}

extern "C" int pdsc_wfrag_build_tail(const float* w1, const float* b1, const float* w2, const float* b2, const float* w3,
                                     const float* b3, void* out, int gemm_format, void* stream) {
    PDSC_REQUIRE(w1 && b1 && w2 && b2 && w3 && b3 && out, "pdsc_wfrag_build_tail: null pointer");
    PDSC_REQUIRE(gemm_format == PDSC_LAYER_GEMM_F32 || gemm_format == PDSC_LAYER_GEMM_H3, "pdsc_wfrag_build_tail: gemm_format=%d", gemm_format);
    hipLaunchKernelGGL(wfrag_tail_kernel<false>, dim3(LW_TAIL_CHUNKS * 8 * 64 / 256), dim3(256), 0, (hipStream_t)stream, w1, b1, w2, b2, w3, b3,
                       nullptr, (float*)out, gemm_format);
    return check_launch("pdsc_wfrag_build_tail");
}

extern "C" int pdsc_wfrag_build_head(const float* wp, const float* bp, const float* wq, const float* bq, void* out,
                                     int gemm_format, void* stream) {
    PDSC_REQUIRE(wp && bp && wq && bq && out, "pdsc_wfrag_build_head: null pointer");
    PDSC_REQUIRE(gemm_format == PDSC_LAYER_GEMM_F32 || gemm_format == PDSC_LAYER_GEMM_H3, "pdsc_wfrag_build_head: gemm_format=%d", gemm_format);
    hipLaunchKernelGGL(wfrag_head_kernel<false>, dim3(LW_HEAD_CHUNKS * 8 * 64 / 256), dim3(256), 0, (hipStream_t)stream, wp, bp, wq, bq,
                       nullptr, (unsigned char*)out, gemm_format);
    return check_launch("pdsc_wfrag_build_head");
}
