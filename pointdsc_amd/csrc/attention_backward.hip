// f-12: backward of the spatial-consistency attention (attention.hip), exact fp32 on the matrix cores, no atomics.
//
//   forward (rows as passed: q' = q log2(e)/sqrt(C)):  x_oi = c_oi <q'_o, k_i>,  P_oi = exp2(x_oi - lse_o),  O_o = sum_i P_oi v_i
//   given dO:   D_o   = <dO_o, O_o>
//               dV_i  = sum_o P_oi dO_o
//               dZ_oi = c_oi P_oi (<dO_o, v_i> - D_o)                   (tail keys and tail queries: 0)
//               dq'_o = ln2 sum_i dZ_oi k_i          dk_i = ln2 sum_o dZ_oi q'_o
//   (d/dx of the natural-log softmax is ln2 d/d(log2-domain logit); the ln2 is applied once, to the finished sums.)
//
// Fixed-order sums and bit-identical repeat calls (DESIGN f-11) give the two-kernel form: no kernel adds into memory another
// workgroup writes.  Both recompute S and P from the forward's row statistic lse = m + log2(l).
// Workgroup count: bs * ceil(N / 128) blocks alone are 128 at the training shape and 40 at 1 x 5000, on 256 CUs, so the tile walk
// of both kernels is split nsplit ways (blockIdx.y, as the forward splits its keys); each split writes its un-scaled partial sums
// and att_bwd_merge_kernel adds them in index order.  nsplit == 1 writes dqkv directly.
//   att_bwd_rowdot_kernel  D[o] = <dO_o, O_o>, one 32-lane group per row.
//   att_bwd_dq_kernel      workgroup = 128 queries (lane = query, the forward's orientation), walks 32-key tiles of K and V:
//                            S^T = K Q^T and dP^T = V dO^T   (the forward's QK shape; Q and dO held in 64 VGPRs each)
//                            dQ^T += K^T dZ^T                  (the forward's PV shape; dZ registers are the B operand as they are)
//   att_bwd_dkv_kernel     workgroup = 128 keys (lane = key; K and V held), walks 32-query tiles of Q and dO:
//                            S = Q K^T and dP = dO V^T,  dV^T += dO^T P,  dK^T += Q^T dZ
//                          compat[o in tile][i in block]: per register one row o, 32 adjacent columns per half wave -- no transpose
//                          and no symmetry assumed; lse and D of the tile's queries ride along in LDS.
// k-slot conventions are those of attention.hip's header.  Every tile is the forward's K image: LDS-DMA, 1 KiB per wave
// instruction, double buffered, XOR-swizzled through the source address (chunk ^= row & 15).  The swizzle permutes chunks inside a
// row, so the same image serves the row-slice reads (S, dP) and the column-slice reads (the accumulating products), which read 32
// different chunks of ONE row per half wave.
#include "pdsc_common.h"
#include "attention_common.h"

namespace pdsc {

constexpr int ABW_BLOCK = 128;                           // queries (dQ) / keys (dKV) per workgroup
constexpr int ABW_TILE = 32;                             // keys (dQ) / queries (dKV) per tile
constexpr int ABW_C = PDSC_CHANNELS;
constexpr int ABW_QKV_LD = 3 * PDSC_CHANNELS;
constexpr int ABW_TILE_FLOATS = ABW_TILE * ABW_C;        // 16 KiB
constexpr float ABW_LN2 = 0.693147180559945309f;

struct AttBwdArgs {
    const float* qkv;        // [bs*N][384]
    const float* compat;     // [bs][N][ld]
    long long ld;
    const float* lse;        // [bs*N]
    const float* msg;        // [bs*N][128]
    const float* dmsg;       // [bs*N][128]
    float* dqkv;             // [bs*N][384]
    float* D;                // [bs*N]   (workspace)
    float* part;             // [bs][nsplit][Npad][384]  per-split partial sums (nsplit > 1), un-scaled
    int N, Npad, nsplit, num_tiles;
};

// D[row] = <dmsg[row], msg[row]>: thread -> (row, 4 channels), butterfly over the row's 32 lanes (a fixed order)
__global__ __launch_bounds__(256) void att_bwd_rowdot_kernel(AttBwdArgs a, long long rows) {
    const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long row = min(gid >> 5, rows - 1);       // whole 32-lane groups stay in the shuffles
    const int c4 = (int)(gid & 31) * 4;
    const f32x4 g = *reinterpret_cast<const f32x4*>(a.dmsg + row * ABW_C + c4);
    const f32x4 o = *reinterpret_cast<const f32x4*>(a.msg + row * ABW_C + c4);
    float d = fmaf(g[3], o[3], fmaf(g[2], o[2], fmaf(g[1], o[1], g[0] * o[0])));
#pragma unroll
    for (int w = 16; w >= 1; w >>= 1) d += __shfl_xor(d, w, 64);
    if (c4 == 0 && (gid >> 5) < rows) a.D[row] = d;
}

// one wave issues its quarter (4 x 1 KiB) of two 32-row tiles (rows r0 .. r0+31 of A and of B, clamped to N-1), both swizzled
__device__ __forceinline__ void issue_tile_pair(const float* __restrict__ abase, int lda, const float* __restrict__ bbase, int ldb,
                                                int r0, int N, float* As, float* Bs, int wave, int lane) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int i = wave * 4 + u;                      // 1-KiB piece: rows 2i, 2i+1
        const int row = 2 * i + (lane >> 5);
        const int cph = lane & 31;                       // physical 16-B chunk inside the LDS row
        const int grow = min(r0 + row, N - 1);           // clamp: tail rows are masked where they are used
        const int col = (cph ^ (row & 15)) << 2;
        __builtin_amdgcn_global_load_lds((gptr_t)(abase + (size_t)grow * lda + col), (lptr_t)(As + i * 256), 16, 0, 0);
        __builtin_amdgcn_global_load_lds((gptr_t)(bbase + (size_t)grow * ldb + col), (lptr_t)(Bs + i * 256), 16, 0, 0);
    }
}

// row slice of a swizzled tile: channels 8q+4h .. +3 of row l31
__device__ __forceinline__ f32x4 tile_row_frag(const float* tile, int l31, int h, int q) {
    return *reinterpret_cast<const f32x4*>(tile + l31 * ABW_C + (((2 * q + h) ^ (l31 & 15)) << 2));
}
// column slice of a swizzled tile: channels 4*l31 .. +3 of row `row`
__device__ __forceinline__ f32x4 tile_col_frag(const float* tile, int l31, int row) {
    return *reinterpret_cast<const f32x4*>(tile + row * ABW_C + ((l31 ^ (row & 15)) << 2));
}

__global__ __launch_bounds__(256) void att_bwd_dq_kernel(AttBwdArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];   // K0 K1 V0 V1, 16 KiB each
    const int t = threadIdx.x, lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int l31 = lane & 31, h = lane >> 5;
    const int qb = blockIdx.x, sp = blockIdx.y, b = blockIdx.z;
    const int N = a.N;
    // key-tile range of this split: tiles [kt0, kt1), never empty (nsplit <= tiles)
    const int per = a.num_tiles / a.nsplit, rem = a.num_tiles % a.nsplit;
    const int kt0 = sp * per + min(sp, rem);
    const int kt1 = kt0 + per + (sp < rem ? 1 : 0);

    const float* qkvb = a.qkv + (size_t)b * N * ABW_QKV_LD;
    const float* kbase = qkvb + ABW_C;
    const float* vbase = qkvb + 2 * ABW_C;
    const int query = qb * ABW_BLOCK + wave * 32 + l31;
    const int qrow = min(query, N - 1);
    const float* crow = a.compat + ((size_t)b * N + qrow) * a.ld + 4 * h;

    issue_tile_pair(kbase, ABW_QKV_LD, vbase, ABW_QKV_LD, kt0 * ABW_TILE, N, lds, lds + 2 * ABW_TILE_FLOATS, wave, lane);
    f32x4 qf[16], gf[16];                                            // this lane's Q and dO fragments
    {
        const float* qsrc = qkvb + (size_t)qrow * ABW_QKV_LD + 4 * h;
        const float* gsrc = a.dmsg + ((size_t)b * N + qrow) * ABW_C + 4 * h;
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            qf[q] = *reinterpret_cast<const f32x4*>(qsrc + 8 * q);
            gf[q] = *reinterpret_cast<const f32x4*>(gsrc + 8 * q);
        }
    }
    const float lse = a.lse[(size_t)b * N + qrow];
    const float Drow = a.D[(size_t)b * N + qrow];
    f32x4 cc[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) cc[g] = *reinterpret_cast<const f32x4*>(crow + kt0 * ABW_TILE + 8 * g);

    f32x16 acc[4];
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[c][r] = 0.f;

    for (int kt = kt0; kt < kt1; ++kt) {
        const int buf = (kt - kt0) & 1;
        const float* Kb = lds + buf * ABW_TILE_FLOATS;
        const float* Vb = lds + (2 + buf) * ABW_TILE_FLOATS;
        // tile kt landed (own LDS-DMA pieces) + everyone finished reading the other buffer
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (kt + 1 < kt1)
            issue_tile_pair(kbase, ABW_QKV_LD, vbase, ABW_QKV_LD, (kt + 1) * ABW_TILE, N, lds + (buf ^ 1) * ABW_TILE_FLOATS,
                            lds + (2 + (buf ^ 1)) * ABW_TILE_FLOATS, wave, lane);

        // ---- S^T = K Q^T,  dP^T = V dO^T: lane = query l31, register r = key (r&3)+8(r>>2)+4h ----
        f32x16 s, dp;
#pragma unroll
        for (int r = 0; r < 16; ++r) s[r] = dp[r] = 0.f;
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const f32x4 ka = tile_row_frag(Kb, l31, h, q);
            const f32x4 va = tile_row_frag(Vb, l31, h, q);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                s = __builtin_amdgcn_mfma_f32_32x32x2f32(ka[e], qf[q][e], s, 0, 0, 0);
                dp = __builtin_amdgcn_mfma_f32_32x32x2f32(va[e], gf[q][e], dp, 0, 0, 0);
            }
        }

        // ---- dZ = c P (dP - D), lane-local ----
        float dz[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float c = cc[r >> 2][r & 3];
            const float p = __builtin_amdgcn_exp2f(c * s[r] - lse);
            dz[r] = c * (p * (dp[r] - Drow));
        }
        if (kt + 1 < kt1) {
#pragma unroll
            for (int g = 0; g < 4; ++g) cc[g] = *reinterpret_cast<const f32x4*>(crow + (kt + 1) * ABW_TILE + 8 * g);
        }
        if ((kt + 1) * ABW_TILE > N) {   // tail tile (wave-uniform branch): keys >= N are not in the softmax
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int key = kt * ABW_TILE + (r & 3) + 8 * (r >> 2) + 4 * h;
                dz[r] = key < N ? dz[r] : 0.f;
            }
        }

        // ---- dQ^T += K^T dZ^T ----
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const f32x4 ka = tile_col_frag(Kb, l31, (r & 3) + 8 * (r >> 2) + 4 * h);
#pragma unroll
            for (int c = 0; c < 4; ++c) acc[c] = __builtin_amdgcn_mfma_f32_32x32x2f32(ka[c], dz[r], acc[c], 0, 0, 0);
        }
    }

    // ---- epilogue: acc[c][r] = dQ^T[channel 4*i+c][query l31], i = (r&3)+8(r>>2)+4h ----
    if (query < N) {
        const float w = a.nsplit == 1 ? ABW_LN2 : 1.0f;              // partials stay un-scaled: the merge applies ln2 to the sum
        float* dst = a.nsplit == 1 ? a.dqkv + ((size_t)b * N + query) * ABW_QKV_LD
                                   : a.part + (((size_t)b * a.nsplit + sp) * a.Npad + query) * ABW_QKV_LD;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int i = (r & 3) + 8 * (r >> 2) + 4 * h;
            f32x4 v = {acc[0][r] * w, acc[1][r] * w, acc[2][r] * w, acc[3][r] * w};
            *reinterpret_cast<f32x4*>(dst + 4 * i) = v;
        }
    }
}

__global__ __launch_bounds__(256) void att_bwd_dkv_kernel(AttBwdArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];   // Q0 Q1 dO0 dO1, 16 KiB each, then (lse | D) x 2 tiles
    const int t = threadIdx.x, lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int l31 = lane & 31, h = lane >> 5;
    const int kb = blockIdx.x, sp = blockIdx.y, b = blockIdx.z;
    const int N = a.N;
    // query-tile range of this split: tiles [qt0, qt1), never empty (nsplit <= tiles)
    const int per = a.num_tiles / a.nsplit, rem = a.num_tiles % a.nsplit;
    const int qt0 = sp * per + min(sp, rem);
    const int qt1 = qt0 + per + (sp < rem ? 1 : 0);
    float* stats = lds + 4 * ABW_TILE_FLOATS;                        // [2][64]: lse of the tile's 32 queries, then their D

    const float* qkvb = a.qkv + (size_t)b * N * ABW_QKV_LD;
    const float* gbase = a.dmsg + (size_t)b * N * ABW_C;
    const int key = kb * ABW_BLOCK + wave * 32 + l31;
    const int krow = min(key, N - 1);
    const float* ccol = a.compat + (size_t)b * N * a.ld + krow;      // column of this lane's key (clamped: ld may end at N rounded to 32)
    const float* stat_src = (h ? a.D : a.lse) + (size_t)b * N;

    // the tile's 32 lse and 32 D: one 4-byte LDS-DMA of wave 0 (lanes 0..31 lse, 32..63 D)
    auto issue_tile = [&](int tile, int buf) {
        issue_tile_pair(qkvb, ABW_QKV_LD, gbase, ABW_C, tile * ABW_TILE, N, lds + buf * ABW_TILE_FLOATS,
                        lds + (2 + buf) * ABW_TILE_FLOATS, wave, lane);
        if (wave == 0)
            __builtin_amdgcn_global_load_lds((gptr_t)(stat_src + min(tile * ABW_TILE + l31, N - 1)), (lptr_t)(stats + buf * 64), 4, 0, 0);
    };
    // compat[o][key] of the tile's queries o = (r&3)+8(r>>2)+4h
    auto load_compat = [&](int tile, float* cc) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int o = min(tile * ABW_TILE + (r & 3) + 8 * (r >> 2) + 4 * h, N - 1);
            cc[r] = ccol[(size_t)o * a.ld];
        }
    };

    issue_tile(qt0, 0);
    f32x4 kf[16], vf[16];                                            // this lane's K and V fragments
    {
        const float* ksrc = qkvb + (size_t)krow * ABW_QKV_LD + ABW_C + 4 * h;
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            kf[q] = *reinterpret_cast<const f32x4*>(ksrc + 8 * q);
            vf[q] = *reinterpret_cast<const f32x4*>(ksrc + ABW_C + 8 * q);
        }
    }
    float cc[16];
    load_compat(qt0, cc);

    f32x16 dk[4], dv[4];
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int r = 0; r < 16; ++r) dk[c][r] = dv[c][r] = 0.f;

    for (int qt = qt0; qt < qt1; ++qt) {
        const int buf = (qt - qt0) & 1;
        const float* Qb = lds + buf * ABW_TILE_FLOATS;
        const float* Gb = lds + (2 + buf) * ABW_TILE_FLOATS;
        const float* st = stats + buf * 64;
        // tile qt landed (own LDS-DMA pieces) + everyone finished reading the other buffer
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (qt + 1 < qt1) issue_tile(qt + 1, buf ^ 1);

        // ---- S = Q K^T,  dP = dO V^T: lane = key l31, register r = query (r&3)+8(r>>2)+4h ----
        f32x16 s, dp;
#pragma unroll
        for (int r = 0; r < 16; ++r) s[r] = dp[r] = 0.f;
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const f32x4 qa = tile_row_frag(Qb, l31, h, q);
            const f32x4 ga = tile_row_frag(Gb, l31, h, q);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                s = __builtin_amdgcn_mfma_f32_32x32x2f32(qa[e], kf[q][e], s, 0, 0, 0);
                dp = __builtin_amdgcn_mfma_f32_32x32x2f32(ga[e], vf[q][e], dp, 0, 0, 0);
            }
        }

        // ---- P and dZ of (query r, key lane) ----
        float p[16], dz[16];
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const f32x4 ls = *reinterpret_cast<const f32x4*>(st + 8 * g + 4 * h);
            const f32x4 Ds = *reinterpret_cast<const f32x4*>(st + 32 + 8 * g + 4 * h);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int r = 4 * g + e;
                p[r] = __builtin_amdgcn_exp2f(cc[r] * s[r] - ls[e]);
                dz[r] = cc[r] * (p[r] * (dp[r] - Ds[e]));
            }
        }
        if (qt + 1 < qt1) load_compat(qt + 1, cc);
        if ((qt + 1) * ABW_TILE > N) {   // tail tile (wave-uniform branch): queries >= N do not exist
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const bool live = qt * ABW_TILE + (r & 3) + 8 * (r >> 2) + 4 * h < N;
                p[r] = live ? p[r] : 0.f;
                dz[r] = live ? dz[r] : 0.f;
            }
        }

        // ---- dV^T += dO^T P,  dK^T += Q^T dZ ----
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int o = (r & 3) + 8 * (r >> 2) + 4 * h;
            const f32x4 ga = tile_col_frag(Gb, l31, o);
            const f32x4 qa = tile_col_frag(Qb, l31, o);
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                dv[c] = __builtin_amdgcn_mfma_f32_32x32x2f32(ga[c], p[r], dv[c], 0, 0, 0);
                dk[c] = __builtin_amdgcn_mfma_f32_32x32x2f32(qa[c], dz[r], dk[c], 0, 0, 0);
            }
        }
    }

    // ---- epilogue: dk[c][r] = dK^T[channel 4*i+c][key l31], i = (r&3)+8(r>>2)+4h ----
    if (key < N) {
        const float w = a.nsplit == 1 ? ABW_LN2 : 1.0f;
        float* dst = (a.nsplit == 1 ? a.dqkv + ((size_t)b * N + key) * ABW_QKV_LD
                                    : a.part + (((size_t)b * a.nsplit + sp) * a.Npad + key) * ABW_QKV_LD) + ABW_C;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int i = (r & 3) + 8 * (r >> 2) + 4 * h;
            f32x4 k4 = {dk[0][r] * w, dk[1][r] * w, dk[2][r] * w, dk[3][r] * w};
            f32x4 v4 = {dv[0][r], dv[1][r], dv[2][r], dv[3][r]};
            *reinterpret_cast<f32x4*>(dst + 4 * i) = k4;
            *reinterpret_cast<f32x4*>(dst + ABW_C + 4 * i) = v4;
        }
    }
}

// dqkv[row] = (ln2 | ln2 | 1) * sum over the splits, in index order: thread -> (row, 4 of the 384 columns)
__global__ __launch_bounds__(256) void att_bwd_merge_kernel(AttBwdArgs a) {
    const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
    const int b = blockIdx.y;
    const long long row = gid / 96;
    const int c4 = (int)(gid % 96) * 4;
    if (row >= a.N) return;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int sp = 0; sp < a.nsplit; ++sp) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(a.part + (((size_t)b * a.nsplit + sp) * a.Npad + row) * ABW_QKV_LD + c4);
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[c] += v[c];
    }
    const float w = c4 < 2 * ABW_C ? ABW_LN2 : 1.0f;
    f32x4 out = {acc[0] * w, acc[1] * w, acc[2] * w, acc[3] * w};
    *reinterpret_cast<f32x4*>(a.dqkv + ((size_t)b * a.N + row) * ABW_QKV_LD + c4) = out;
}

static int abw_npad(int N) { return (int)round_up(N, ABW_BLOCK); }
static int abw_effective_split(int bs, int N, int nsplit) {
    const int tiles = ceil_div(N, ABW_TILE);
    if (nsplit <= 0) nsplit = pdsc_attention_backward_default_split(bs, N);
    return nsplit > tiles ? tiles : nsplit;
}

}  // namespace pdsc

extern "C" int pdsc_attention_backward_default_split(int bs, int N) {
    if (bs <= 0 || N <= 0) return -1;
    const int blocks = pdsc::ceil_div(N, pdsc::ABW_BLOCK) * bs;
    const int tiles = pdsc::ceil_div(N, pdsc::ABW_TILE);
    // both kernels run one wave per SIMD (more than 256 registers), so one workgroup per CU: aim for ~256, keep >= 4 tiles each
    int ns = (256 + blocks / 2) / blocks;
    if (ns < 1) ns = 1;
    const int cap = tiles / 4 > 1 ? tiles / 4 : 1;
    return ns > cap ? cap : ns;
}

extern "C" size_t pdsc_attention_backward_split_workspace_bytes(int bs, int N, int nsplit) {
    if (bs <= 0 || N <= 0) return 0;
    nsplit = pdsc::abw_effective_split(bs, N, nsplit);
    const size_t d_floats = (size_t)pdsc::round_up((long long)bs * N, 4);      // D, then the partials on a 16-byte boundary
    const size_t part_floats = nsplit > 1 ? (size_t)bs * nsplit * pdsc::abw_npad(N) * pdsc::ABW_QKV_LD : 0;
    return (d_floats + part_floats) * sizeof(float);
}

extern "C" size_t pdsc_attention_backward_workspace_bytes(int bs, int N) {
    return pdsc_attention_backward_split_workspace_bytes(bs, N, 0);
}

extern "C" int pdsc_sc_attention_backward_split(const float* qkv, const float* compat, long long ld, const float* msg, const float* lse,
                                                const float* dmsg, float* dqkv, void* workspace, size_t workspace_bytes, int bs, int N,
                                                int nsplit, void* stream) {
    PDSC_REQUIRE(qkv && compat && msg && lse && dmsg && dqkv && workspace, "pdsc_sc_attention_backward: null pointer");
    PDSC_REQUIRE(bs > 0 && N > 0, "pdsc_sc_attention_backward: bs=%d N=%d", bs, N);
    PDSC_REQUIRE(ld >= pdsc::round_up(N, pdsc::ABW_TILE) && ld % 4 == 0,
                 "pdsc_sc_attention_backward: ld=%lld must be a multiple of 4 and >= N rounded up to 32", ld);
    nsplit = pdsc::abw_effective_split(bs, N, nsplit);
    const size_t need = pdsc_attention_backward_split_workspace_bytes(bs, N, nsplit);
    if (workspace_bytes < need) {
        pdsc::set_error("pdsc_sc_attention_backward: workspace %zu < %zu bytes", workspace_bytes, need);
        return PDSC_ERR_WORKSPACE;
    }
    pdsc::AttBwdArgs a{};
    a.qkv = qkv; a.compat = compat; a.ld = ld; a.lse = lse; a.msg = msg; a.dmsg = dmsg; a.dqkv = dqkv;
    a.D = (float*)workspace;
    a.part = a.D + pdsc::round_up((long long)bs * N, 4);
    a.N = N; a.Npad = pdsc::abw_npad(N); a.nsplit = nsplit; a.num_tiles = pdsc::ceil_div(N, pdsc::ABW_TILE);
    hipStream_t st = (hipStream_t)stream;
    const size_t dq_lds = 4 * pdsc::ABW_TILE_FLOATS * sizeof(float);                 // 64 KiB
    const size_t dkv_lds = dq_lds + 2 * 64 * sizeof(float);
    int rc = pdsc::ensure_dynamic_lds(reinterpret_cast<const void*>(&pdsc::att_bwd_dq_kernel), dq_lds, "pdsc_sc_attention_backward(dynamic LDS)");
    if (rc != PDSC_OK) return rc;
    rc = pdsc::ensure_dynamic_lds(reinterpret_cast<const void*>(&pdsc::att_bwd_dkv_kernel), dkv_lds, "pdsc_sc_attention_backward(dynamic LDS)");
    if (rc != PDSC_OK) return rc;

    const long long rows = (long long)bs * N;
    hipLaunchKernelGGL(pdsc::att_bwd_rowdot_kernel, dim3((unsigned)((rows * 32 + 255) / 256)), dim3(256), 0, st, a, rows);
    rc = pdsc::check_launch("pdsc_sc_attention_backward(row dot)");
    if (rc != PDSC_OK) return rc;
    const dim3 grid(pdsc::ceil_div(N, pdsc::ABW_BLOCK), nsplit, bs);
    hipLaunchKernelGGL(pdsc::att_bwd_dq_kernel, grid, dim3(256), dq_lds, st, a);
    rc = pdsc::check_launch("pdsc_sc_attention_backward(dq)");
    if (rc != PDSC_OK) return rc;
    hipLaunchKernelGGL(pdsc::att_bwd_dkv_kernel, grid, dim3(256), dkv_lds, st, a);
    rc = pdsc::check_launch("pdsc_sc_attention_backward(dkv)");
    if (rc != PDSC_OK || nsplit == 1) return rc;
    hipLaunchKernelGGL(pdsc::att_bwd_merge_kernel, dim3((unsigned)(((long long)N * 96 + 255) / 256), bs), dim3(256), 0, st, a);
    return pdsc::check_launch("pdsc_sc_attention_backward(merge)");
}

extern "C" int pdsc_sc_attention_backward(const float* qkv, const float* compat, long long ld, const float* msg, const float* lse,
                                          const float* dmsg, float* dqkv, void* workspace, size_t workspace_bytes, int bs, int N,
                                          void* stream) {
    return pdsc_sc_attention_backward_split(qkv, compat, ld, msg, lse, dmsg, dqkv, workspace, workspace_bytes, bs, N, 0, stream);
}
