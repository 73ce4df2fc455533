// f-16: the train path's plain linears, forward and backward on channel-last rows: layer0 and
// fc_message.6 with its residual (pdsc_linear_train_*), the q|k|v projection (pdsc_qkv_train_*) and the classification head
// (pdsc_head_train_*).  Reference: models/PointDSC.py:36-45,65-77,171 under model.train().
//
//   linear   Y = X W^T + b (+ R);                       dX = dY W;  dW = dY^T X;  db = sum_rows dY      (dR is dY itself)
//   q|k|v    qkv = (s (X Wq^T + bq) | X Wk^T + bk | X Wv^T + bv): the scale s is applied to the PRODUCT, after the bias;
//            backward on g = (s dq | dk | dv), rounded once:  dX = g_q Wq + g_k Wk + g_v Wv;  dW_p = g_p^T X;  db_p = sum_rows g_p
//            -- the gradients of the un-scaled parameters
//   head     A0 = X W0^T + b0;  A1 = relu(A0) W1^T + b1;  logits = relu(A1) . w2 + b2                    (128 -> 32 -> 32 -> 1)
//            backward: A0, A1 recomputed by the forward's own function (lth_hidden), masks A1 > 0, A0 > 0 from them, no mask stored
//
// Structure of pointwise_train.hip: v_mfma_f32_32x32x2_f32 (exact fp32 products), 64-row tiles, the whole K in LDS behind
// linear.hip's row pad of 4, operand convention k-slot (step 4q+e, half h = lane>>5) <-> channel 8q+4h+e.  The backward's parameter
// gradients are accumulated in registers by persistent workgroups (at most LT_MAX_GROUPS) over the tiles they walk, written as one
// partial per workgroup and added in index order by lt_merge_kernel: no atomics, no memset, nothing allocated, every sum in a fixed
// order.  dX and dW come from two independent kernels (lt_dx_kernel, lt_dw_kernel), so an output that is not wanted costs nothing
// and the others keep their bits.
#include "pdsc_common.h"

namespace pdsc {

constexpr int LT_BM = 64;                  // rows per tile
constexpr int LT_C = 128;                  // output channels of every linear here (per part of q|k|v)
constexpr int LT_LDO = LT_C + 4;
constexpr int LT_MAX_GROUPS = 256;         // persistent workgroups of the backward kernels: one per compute unit
constexpr int LT_MERGE_THREADS = 1024;

static int lt_tiles(int M) { return ceil_div(M, LT_BM); }
static int lt_groups(int M) { const int t = lt_tiles(M); return t < LT_MAX_GROUPS ? t : LT_MAX_GROUPS; }
static bool lt_shape_ok(int Cin, int Cout) { return Cout == LT_C && ((Cin >= 1 && Cin <= 16) || Cin == 64); }

// ---- forward: one workgroup per (64-row tile, part): Y[:, part 128 ..] = (X W_part^T + b_part) s_part (+ R) ------------------
struct LtFwdArgs {
    const float* X; const float* W0; const float* W1; const float* W2; const float* b0; const float* b1; const float* b2;
    const float* R; float* Y;
    float scale0;                // of part 0; the other parts are not scaled
    int M, Cin, ldy;
};

// CINP: K as staged (Cin padded with zeros); VEC: 16-byte global loads of X and W (Cin a multiple of 4, CINP == Cin)
template <int CINP>
__global__ __launch_bounds__(256) void lt_forward_kernel(LtFwdArgs a) {
    constexpr int KP = CINP + 4, K4 = CINP / 4, NT = LT_C / 64;
    constexpr bool VEC = CINP >= 64;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float* Xs = lds;                       // [64][KP]
    float* Ws = lds + LT_BM * KP;          // [128][KP]
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int part = blockIdx.y;
    const int m0 = blockIdx.x * LT_BM;
    const int nrows = min(LT_BM, a.M - m0);
    const float* W = part == 0 ? a.W0 : (part == 1 ? a.W1 : a.W2);
    const float* b = part == 0 ? a.b0 : (part == 1 ? a.b1 : a.b2);
    const float sc = part == 0 ? a.scale0 : 1.f;

    if (VEC) {
        for (int idx = t; idx < LT_BM * K4; idx += 256) {
            const int row = idx / K4, c = idx - row * K4;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (row < nrows) v = *reinterpret_cast<const f32x4*>(a.X + (size_t)(m0 + row) * CINP + c * 4);
            *reinterpret_cast<f32x4*>(Xs + row * KP + c * 4) = v;
        }
        for (int idx = t; idx < LT_C * K4; idx += 256) {
            const int row = idx / K4, c = idx - row * K4;
            *reinterpret_cast<f32x4*>(Ws + row * KP + c * 4) = *reinterpret_cast<const f32x4*>(W + (size_t)row * CINP + c * 4);
        }
    } else {
        for (int idx = t; idx < LT_BM * CINP; idx += 256) {
            const int row = idx / CINP, c = idx - row * CINP;
            Xs[row * KP + c] = (row < nrows && c < a.Cin) ? a.X[(size_t)(m0 + row) * a.Cin + c] : 0.f;
        }
        for (int idx = t; idx < LT_C * CINP; idx += 256) {
            const int row = idx / CINP, c = idx - row * CINP;
            Ws[row * KP + c] = c < a.Cin ? W[(size_t)row * a.Cin + c] : 0.f;
        }
    }
    __syncthreads();

    const int wm = wave & 1, wn = wave >> 1;
    const int l31 = lane & 31, h = lane >> 5;
    f32x16 acc[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[nt][r] = 0.f;
    const float* xa = Xs + (wm * 32 + l31) * KP + 4 * h;
    const float* wb = Ws + ((wn * NT) * 32 + l31) * KP + 4 * h;
#pragma unroll 2
    for (int q = 0; q < CINP / 8; ++q) {
        const f32x4 av = *reinterpret_cast<const f32x4*>(xa + 8 * q);
        f32x4 bv[NT];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) bv[nt] = *reinterpret_cast<const f32x4*>(wb + nt * 32 * KP + 8 * q);
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
                acc[nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[e], bv[nt][e], acc[nt], 0, 0, 0);
    }

#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        const int n = (wn * NT + nt) * 32 + l31;
        const float bval = b[n];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int i = wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
            if (i < nrows) {
                float v = (acc[nt][r] + bval) * sc;
                if (a.R) v += a.R[(size_t)(m0 + i) * LT_C + n];
                a.Y[(size_t)(m0 + i) * a.ldy + part * LT_C + n] = v;
            }
        }
    }
}

struct LtBwdArgs {
    const float* dY; const float* X; const float* W0; const float* W1; const float* W2;
    float* dX; float* part;      // part [parts][groups][128 * Cin + 128]
    float scale0;
    int M, Cin, ldy;
};

// the dY tile of one part -> LDS [64][LT_LDO], part 0 times scale0 (one rounding), rows past the end zero; thread = 4 channels of
// a row, rows rl, rl + 8, ...; dbs += the thread's column sums when SUM
template <bool SUM>
__device__ __forceinline__ void lt_stage_dy(const LtBwdArgs& a, float* dYs, int m0, int nrows, int p, float (&dbs)[4]) {
    const int t = threadIdx.x, c4 = (t & 31) * 4, rl = t >> 5;
    const float sc = p == 0 ? a.scale0 : 1.f;
#pragma unroll
    for (int i = 0; i < LT_BM / 8; ++i) {
        const int r = rl + 8 * i;
        f32x4 dy = {0.f, 0.f, 0.f, 0.f};
        if (r < nrows) {
            dy = *reinterpret_cast<const f32x4*>(a.dY + (size_t)(m0 + r) * a.ldy + p * LT_C + c4);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                dy[e] *= sc;
                if (SUM) dbs[e] += dy[e];
            }
        }
        *reinterpret_cast<f32x4*>(dYs + r * LT_LDO + c4) = dy;
    }
}

// rows [rows][Cin] of global memory -> LDS [rows][CIS + 4], columns Cin .. CIS - 1 and rows >= nvalid zero
template <int CIS>
__device__ __forceinline__ void lt_stage_rows(const float* __restrict__ src, float* dst, int rows, int nvalid, int Cin) {
    constexpr int LDI = CIS + 4, K4 = CIS / 4;
    const int t = threadIdx.x;
    if (CIS >= 64) {
        for (int idx = t; idx < rows * K4; idx += 256) {
            const int row = idx / K4, c = idx - row * K4;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (row < nvalid) v = *reinterpret_cast<const f32x4*>(src + (size_t)row * CIS + c * 4);
            *reinterpret_cast<f32x4*>(dst + row * LDI + c * 4) = v;
        }
    } else {
        for (int idx = t; idx < rows * CIS; idx += 256) {
            const int row = idx / CIS, c = idx - row * CIS;
            dst[row * LDI + c] = (row < nvalid && c < Cin) ? src[(size_t)row * Cin + c] : 0.f;
        }
    }
}

// ---- backward, dX: persistent workgroups walk the tiles; dX tile = sum over the parts of dY_p W_p --------------------------
// CIS: Cin as staged (32 for Cin <= 16: the matrix instruction's N is 32; 64; 128).  PARTS == 1: W staged once per workgroup.
template <int CIS, int PARTS>
__global__ __launch_bounds__(256) void lt_dx_kernel(LtBwdArgs a) {
    constexpr int LDI = CIS + 4;
    constexpr int NTI = CIS >= 64 ? CIS / 64 : 1;            // 32-column blocks per wave
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float* dYs = lds;                                        // [64][LT_LDO]
    float* Ws = dYs + LT_BM * LT_LDO;                        // [128][LDI]
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, l31 = lane & 31, h = lane >> 5;
    const int wm = wave & 1, wn = wave >> 1;
    const bool active = wn * NTI * 32 < CIS;                 // CIS == 32: two of the four waves own the 64 x 32 tile
    const int tiles = ceil_div_dev(a.M, LT_BM);
    float unused[4] = {0.f, 0.f, 0.f, 0.f};

    if (PARTS == 1) lt_stage_rows<CIS>(a.W0, Ws, LT_C, LT_C, a.Cin);
    for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int m0 = tile * LT_BM;
        const int nrows = min(LT_BM, a.M - m0);
        f32x16 acc[NTI];
#pragma unroll
        for (int nt = 0; nt < NTI; ++nt)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[nt][r] = 0.f;
#pragma unroll 1
        for (int p = 0; p < PARTS; ++p) {
            __syncthreads();                                 // the previous readers are done
            lt_stage_dy<false>(a, dYs, m0, nrows, p, unused);
            if (PARTS > 1) lt_stage_rows<CIS>(p == 0 ? a.W0 : (p == 1 ? a.W1 : a.W2), Ws, LT_C, LT_C, a.Cin);
            __syncthreads();
            if (active) {
                // dX[m][ci] += sum_co dY[m][co] W[co][ci]: A = dY rows (one 16-byte read per four steps), B = W rows (k = co)
                const float* ya = dYs + (wm * 32 + l31) * LT_LDO + 4 * h;
                const float* wb = Ws + (4 * h) * LDI + wn * NTI * 32 + l31;
#pragma unroll 2
                for (int q = 0; q < LT_C / 8; ++q) {
                    const f32x4 av = *reinterpret_cast<const f32x4*>(ya + 8 * q);
#pragma unroll
                    for (int e = 0; e < 4; ++e)
#pragma unroll
                        for (int nt = 0; nt < NTI; ++nt)
                            acc[nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[e], wb[(8 * q + e) * LDI + nt * 32], acc[nt], 0, 0, 0);
                }
            }
        }
        if (active) {
#pragma unroll
            for (int nt = 0; nt < NTI; ++nt) {
                const int n = (wn * NTI + nt) * 32 + l31;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int i = wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
                    if (i < nrows && n < a.Cin) a.dX[(size_t)(m0 + i) * a.Cin + n] = acc[nt][r];
                }
            }
        }
    }
}

// ---- backward, dW and db: workgroup (g, p) walks the tiles g, g + groups, ... of part p: dW_p += dY_p^T X, db_p += sum dY_p ---
template <int CIS>
__global__ __launch_bounds__(256) void lt_dw_kernel(LtBwdArgs a) {
    constexpr int LDI = CIS + 4;
    constexpr int CIB = CIS / 32, TPW = CIB;                 // 32 x 32 blocks of dW: 4 x CIB, TPW per wave
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float* dYs = lds;                                        // [64][LT_LDO]
    float* Xs = dYs + LT_BM * LT_LDO;                        // [64][LDI]
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, l31 = lane & 31, h = lane >> 5;
    const int c4 = (t & 31) * 4, rl = t >> 5;
    const int p = blockIdx.y;
    const int tiles = ceil_div_dev(a.M, LT_BM);
    float dbs[4] = {0.f, 0.f, 0.f, 0.f};
    f32x16 accw[TPW];
#pragma unroll
    for (int i = 0; i < TPW; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) accw[i][r] = 0.f;

    for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int m0 = tile * LT_BM;
        const int nrows = min(LT_BM, a.M - m0);
        __syncthreads();
        lt_stage_dy<true>(a, dYs, m0, nrows, p, dbs);
        lt_stage_rows<CIS>(a.X + (size_t)m0 * a.Cin, Xs, LT_BM, nrows, a.Cin);
        __syncthreads();
        // dW[co][ci] += sum_rows dY[row][co] X[row][ci]: k = row 2 step + h, both operands one 4-byte read per step
#pragma unroll 4
        for (int st = 0; st < LT_BM / 2; ++st) {
            const float* yr = dYs + (2 * st + h) * LT_LDO + l31;
            const float* xr = Xs + (2 * st + h) * LDI + l31;
#pragma unroll
            for (int i = 0; i < TPW; ++i) {
                const int j = wave * TPW + i;                // block (co, ci) = (j / CIB, j % CIB)
                accw[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(yr[(j / CIB) * 32], xr[(j % CIB) * 32], accw[i], 0, 0, 0);
            }
        }
    }

    const int per = LT_C * a.Cin + LT_C;
    float* P = a.part + ((size_t)p * gridDim.x + blockIdx.x) * per;
#pragma unroll
    for (int i = 0; i < TPW; ++i) {
        const int j = wave * TPW + i;
        const int ci = (j % CIB) * 32 + l31;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int co = (j / CIB) * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
            if (ci < a.Cin) P[(size_t)co * a.Cin + ci] = accw[i][r];
        }
    }
    // db: the row lanes of a channel in order
    __syncthreads();
    float* red = dYs;                                        // [8][128]
#pragma unroll
    for (int e = 0; e < 4; ++e) red[rl * LT_C + c4 + e] = dbs[e];
    __syncthreads();
    if (t < LT_C) {
        float s = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) s += red[j * LT_C + t];
        P[LT_C * a.Cin + t] = s;
    }
}

// ---- the workgroups' partials in index order -> the caller's tensors -----------------------------------------------------------
// part [sets = gridDim.y][groups][total]; element el of set y goes to the segment k with set[k] == y and begin[k] <= el < end[k]
// (a NULL out[k]: not wanted).  thread = (slice, element), 16 slices x 64 elements, as pwt_merge_dw_kernel.
constexpr int LT_MAX_SEGS = 6;
struct LtMergeSegs {
    int set[LT_MAX_SEGS], begin[LT_MAX_SEGS], end[LT_MAX_SEGS];
    float* out[LT_MAX_SEGS];
};

__global__ __launch_bounds__(LT_MERGE_THREADS) void lt_merge_kernel(const float* __restrict__ part, int groups, int total, LtMergeSegs sg) {
    __shared__ float red[LT_MERGE_THREADS];
    const int t = threadIdx.x, el = blockIdx.x * 64 + (t & 63), s = t >> 6, y = blockIdx.y;
    const float* base = part + (size_t)y * groups * total;
    float acc = 0.f;
    if (el < total)
        for (int p = s; p < groups; p += 16) acc += base[(size_t)p * total + el];
    red[t] = acc;
    __syncthreads();
    if (s == 0 && el < total) {
        float tot = 0.f;
#pragma unroll
        for (int j = 0; j < 16; ++j) tot += red[j * 64 + (t & 63)];
#pragma unroll
        for (int k = 0; k < LT_MAX_SEGS; ++k)
            if (sg.set[k] == y && el >= sg.begin[k] && el < sg.end[k] && sg.out[k]) sg.out[k][el - sg.begin[k]] = tot;
    }
}

// ---- the classification head ---------------------------------------------------------------------------------------------------
constexpr int LTH_CIN = 128, LTH_H = 32;
constexpr int LTH_LDX = LTH_CIN + 4;       // X tile and W0 rows
constexpr int LTH_LDH = LTH_H + 4;         // W1 rows, A0, dA0, dA1 (16-byte reads along a row)
constexpr int LTH_LDA = LTH_H + 1;         // A1 (read along columns by a thread per row)
// partial of a backward workgroup: dW0 [32][128] | db0 [32] | dW1 [32][32] | db1 [32] | dW2 [32] | db2
constexpr int LTH_O_DB0 = LTH_H * LTH_CIN, LTH_O_DW1 = LTH_O_DB0 + LTH_H, LTH_O_DB1 = LTH_O_DW1 + LTH_H * LTH_H,
              LTH_O_DW2 = LTH_O_DB1 + LTH_H, LTH_O_DB2 = LTH_O_DW2 + LTH_H, LTH_PART = LTH_O_DB2 + 1;

struct LthLds {
    float* Xs;       // [64][LTH_LDX]
    float* W0s;      // [32][LTH_LDX]
    float* W1s;      // [32][LTH_LDH]
    float* A0s;      // [64][LTH_LDH]  pre-activation of the first hidden layer
    float* A1s;      // [64][LTH_LDA]  pre-activation of the second
    float* b0s; float* b1s; float* w2s;      // [32] each
};
constexpr int LTH_FWD_FLOATS = LT_BM * LTH_LDX + LTH_H * LTH_LDX + LTH_H * LTH_LDH + LT_BM * LTH_LDH + LT_BM * LTH_LDA + 3 * LTH_H;

__device__ __forceinline__ LthLds lth_carve(float* lds) {
    LthLds s;
    s.Xs = lds;
    s.W0s = s.Xs + LT_BM * LTH_LDX;
    s.W1s = s.W0s + LTH_H * LTH_LDX;
    s.A0s = s.W1s + LTH_H * LTH_LDH;
    s.A1s = s.A0s + LT_BM * LTH_LDH;
    s.b0s = s.A1s + LT_BM * LTH_LDA;
    s.b1s = s.b0s + LTH_H;
    s.w2s = s.b1s + LTH_H;
    return s;
}

struct LthArgs {
    const float* X; const float* W0; const float* b0; const float* W1; const float* b1; const float* W2; const float* b2;
    const float* dL;             // backward: dlogits [M]
    float* logits; float* pre; float* dX; float* part;      // pre: the forward's optional [M][64] = (A0 | A1)
    int M;
};

__device__ __forceinline__ void lth_stage_weights(const LthArgs& a, const LthLds& s) {
    const int t = threadIdx.x;
    for (int idx = t; idx < LTH_H * (LTH_CIN / 4); idx += 256) {
        const int row = idx / (LTH_CIN / 4), c = idx - row * (LTH_CIN / 4);
        *reinterpret_cast<f32x4*>(s.W0s + row * LTH_LDX + c * 4) = *reinterpret_cast<const f32x4*>(a.W0 + (size_t)row * LTH_CIN + c * 4);
    }
    for (int idx = t; idx < LTH_H * LTH_H; idx += 256) s.W1s[(idx >> 5) * LTH_LDH + (idx & 31)] = a.W1[idx];
    if (t < LTH_H) { s.b0s[t] = a.b0[t]; s.b1s[t] = a.b1[t]; s.w2s[t] = a.W2[t]; }
}

__device__ __forceinline__ void lth_stage_x(const LthArgs& a, const LthLds& s, int m0, int nrows) {
    for (int idx = threadIdx.x; idx < LT_BM * (LTH_CIN / 4); idx += 256) {
        const int row = idx / (LTH_CIN / 4), c = idx - row * (LTH_CIN / 4);
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (row < nrows) v = *reinterpret_cast<const f32x4*>(a.X + (size_t)(m0 + row) * LTH_CIN + c * 4);
        *reinterpret_cast<f32x4*>(s.Xs + row * LTH_LDX + c * 4) = v;
    }
}

// A0 = X W0^T + b0, A1 = relu(A0) W1^T + b1 of the staged tile; the forward and the backward both call THIS, so the backward's
// masks A0 > 0, A1 > 0 are the forward's bits.  Waves 0 and 1 own 32 rows each (a 32 x 32 output block); ends with a barrier.
__device__ __forceinline__ void lth_hidden(const LthLds& s) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l31 = lane & 31, h = lane >> 5;
    __syncthreads();                                         // the stage is complete
    if (wave < 2) {
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
        const float* xa = s.Xs + (wave * 32 + l31) * LTH_LDX + 4 * h;
        const float* wb = s.W0s + l31 * LTH_LDX + 4 * h;
#pragma unroll 4
        for (int q = 0; q < LTH_CIN / 8; ++q) {
            const f32x4 av = *reinterpret_cast<const f32x4*>(xa + 8 * q);
            const f32x4 bv = *reinterpret_cast<const f32x4*>(wb + 8 * q);
#pragma unroll
            for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[e], bv[e], acc, 0, 0, 0);
        }
        const float bval = s.b0s[l31];
#pragma unroll
        for (int r = 0; r < 16; ++r) s.A0s[(wave * 32 + (r & 3) + 8 * (r >> 2) + 4 * h) * LTH_LDH + l31] = acc[r] + bval;
    }
    __syncthreads();
    if (wave < 2) {
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
        const float* xa = s.A0s + (wave * 32 + l31) * LTH_LDH + 4 * h;
        const float* wb = s.W1s + l31 * LTH_LDH + 4 * h;
#pragma unroll
        for (int q = 0; q < LTH_H / 8; ++q) {
            const f32x4 av = *reinterpret_cast<const f32x4*>(xa + 8 * q);
            const f32x4 bv = *reinterpret_cast<const f32x4*>(wb + 8 * q);
#pragma unroll
            for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(fmaxf(av[e], 0.f), bv[e], acc, 0, 0, 0);
        }
        const float bval = s.b1s[l31];
#pragma unroll
        for (int r = 0; r < 16; ++r) s.A1s[(wave * 32 + (r & 3) + 8 * (r >> 2) + 4 * h) * LTH_LDA + l31] = acc[r] + bval;
    }
    __syncthreads();
}

__global__ __launch_bounds__(256) void lth_forward_kernel(LthArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const LthLds s = lth_carve(lds);
    const int t = threadIdx.x;
    const int m0 = blockIdx.x * LT_BM;
    const int nrows = min(LT_BM, a.M - m0);
    lth_stage_weights(a, s);
    lth_stage_x(a, s, m0, nrows);
    lth_hidden(s);
    if (t < nrows) {
        float v = 0.f;
#pragma unroll
        for (int j = 0; j < LTH_H; ++j) v = fmaf(fmaxf(s.A1s[t * LTH_LDA + j], 0.f), s.w2s[j], v);
        a.logits[m0 + t] = v + a.b2[0];
    }
    if (a.pre) {
        for (int idx = t; idx < nrows * 2 * LTH_H; idx += 256) {
            const int row = idx / (2 * LTH_H), c = idx - row * (2 * LTH_H);
            a.pre[(size_t)(m0 + row) * (2 * LTH_H) + c] = c < LTH_H ? s.A0s[row * LTH_LDH + c] : s.A1s[row * LTH_LDA + c - LTH_H];
        }
    }
}

// backward: persistent workgroups walk the tiles.  Per tile: A0, A1 (lth_hidden); dA1 = [A1 > 0] dL w2; dA0 = [A0 > 0] dA1 W1;
// dX = dA0 W0 (DX); dW0 += dA0^T X, dW1 += dA1^T relu(A0), dW2 += dL relu(A1), db0 += sum dA0, db1 += sum dA1, db2 += sum dL (DW)
template <bool DX, bool DW>
__global__ __launch_bounds__(256) void lth_backward_kernel(LthArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const LthLds s = lth_carve(lds);
    float* G0s = lds + LTH_FWD_FLOATS;                       // dA0 [64][LTH_LDH]
    float* G1s = G0s + LT_BM * LTH_LDH;                      // dA1 [64][LTH_LDH]
    float* dLs = G1s + LT_BM * LTH_LDH;                      // [64]
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, l31 = lane & 31, h = lane >> 5;
    const int j = t & 31, rl = t >> 5;                       // element-wise passes: thread = column j of rows rl, rl + 8, ...
    const int tiles = ceil_div_dev(a.M, LT_BM);
    float sdb0 = 0.f, sdb1 = 0.f, sdw2 = 0.f, sdl = 0.f;
    f32x16 accw0, accw1;
#pragma unroll
    for (int r = 0; r < 16; ++r) { accw0[r] = 0.f; accw1[r] = 0.f; }

    lth_stage_weights(a, s);
    for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int m0 = tile * LT_BM;
        const int nrows = min(LT_BM, a.M - m0);
        __syncthreads();                                     // the previous tile's readers are done
        lth_stage_x(a, s, m0, nrows);
        if (t < LT_BM) dLs[t] = t < nrows ? a.dL[m0 + t] : 0.f;
        lth_hidden(s);

        const float w2 = s.w2s[j];
#pragma unroll
        for (int i = 0; i < LT_BM / 8; ++i) {
            const int r = rl + 8 * i;
            const float a1 = s.A1s[r * LTH_LDA + j], dl = dLs[r];
            const float g = a1 > 0.f ? dl * w2 : 0.f;
            G1s[r * LTH_LDH + j] = g;
            sdb1 += g;
            sdw2 = fmaf(dl, fmaxf(a1, 0.f), sdw2);
            sdl += dl;
        }
        __syncthreads();
        if (wave < 2) {
            // dH0[m][j0] = sum_j1 dA1[m][j1] W1[j1][j0]
            f32x16 acc;
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = 0.f;
            const float* ya = G1s + (wave * 32 + l31) * LTH_LDH + 4 * h;
            const float* wb = s.W1s + (4 * h) * LTH_LDH + l31;
#pragma unroll
            for (int q = 0; q < LTH_H / 8; ++q) {
                const f32x4 av = *reinterpret_cast<const f32x4*>(ya + 8 * q);
#pragma unroll
                for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[e], wb[(8 * q + e) * LTH_LDH], acc, 0, 0, 0);
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int i = wave * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
                G0s[i * LTH_LDH + l31] = s.A0s[i * LTH_LDH + l31] > 0.f ? acc[r] : 0.f;
            }
        }
        __syncthreads();

        if (DX) {
            // dX[m][ci] = sum_j0 dA0[m][j0] W0[j0][ci]
            const int wm = wave & 1, wn = wave >> 1;
            f32x16 acc[2];
#pragma unroll
            for (int nt = 0; nt < 2; ++nt)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[nt][r] = 0.f;
            const float* ya = G0s + (wm * 32 + l31) * LTH_LDH + 4 * h;
            const float* wb = s.W0s + (4 * h) * LTH_LDX + wn * 64 + l31;
#pragma unroll
            for (int q = 0; q < LTH_H / 8; ++q) {
                const f32x4 av = *reinterpret_cast<const f32x4*>(ya + 8 * q);
#pragma unroll
                for (int e = 0; e < 4; ++e)
#pragma unroll
                    for (int nt = 0; nt < 2; ++nt)
                        acc[nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[e], wb[(8 * q + e) * LTH_LDX + nt * 32], acc[nt], 0, 0, 0);
            }
#pragma unroll
            for (int nt = 0; nt < 2; ++nt) {
                const int n = wn * 64 + nt * 32 + l31;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int i = wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
                    if (i < nrows) a.dX[(size_t)(m0 + i) * LTH_CIN + n] = acc[nt][r];
                }
            }
        }
        if (DW) {
#pragma unroll
            for (int i = 0; i < LT_BM / 8; ++i) sdb0 += G0s[(rl + 8 * i) * LTH_LDH + j];
            // dW0[j0][ci] += sum_rows dA0[row][j0] X[row][ci]: wave = 32-column block of ci; k = row 2 step + h
#pragma unroll 4
            for (int st = 0; st < LT_BM / 2; ++st)
                accw0 = __builtin_amdgcn_mfma_f32_32x32x2f32(G0s[(2 * st + h) * LTH_LDH + l31], s.Xs[(2 * st + h) * LTH_LDX + wave * 32 + l31],
                                                             accw0, 0, 0, 0);
            // dW1[j1][j0] += sum_rows dA1[row][j1] relu(A0[row][j0]): one block, wave 3 (rows past the end: dA1 = 0)
            if (wave == 3) {
#pragma unroll 4
                for (int st = 0; st < LT_BM / 2; ++st)
                    accw1 = __builtin_amdgcn_mfma_f32_32x32x2f32(G1s[(2 * st + h) * LTH_LDH + l31],
                                                                 fmaxf(s.A0s[(2 * st + h) * LTH_LDH + l31], 0.f), accw1, 0, 0, 0);
            }
        }
    }

    if (DW) {
        float* P = a.part + (size_t)blockIdx.x * LTH_PART;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = (r & 3) + 8 * (r >> 2) + 4 * h;
            P[(size_t)row * LTH_CIN + wave * 32 + l31] = accw0[r];
            if (wave == 3) P[LTH_O_DW1 + row * LTH_H + l31] = accw1[r];
        }
        // the element-wise sums: the row lanes of a column in order
        __syncthreads();
        float* red = G0s;                                    // [4][8][32]
        red[(0 * 8 + rl) * 32 + j] = sdb0;
        red[(1 * 8 + rl) * 32 + j] = sdb1;
        red[(2 * 8 + rl) * 32 + j] = sdw2;
        red[(3 * 8 + rl) * 32 + j] = sdl;
        __syncthreads();
        if (t < 4 * 32) {
            const int which = t >> 5;
            float v = 0.f;
#pragma unroll
            for (int k = 0; k < 8; ++k) v += red[(which * 8 + k) * 32 + j];
            if (which == 0) P[LTH_O_DB0 + j] = v;
            else if (which == 1) P[LTH_O_DB1 + j] = v;
            else if (which == 2) P[LTH_O_DW2 + j] = v;
            else if (j == 0) P[LTH_O_DB2] = v;
        }
    }
}
constexpr int LTH_BWD_FLOATS = LTH_FWD_FLOATS + 2 * LT_BM * LTH_LDH + LT_BM;

// ---- launchers -------------------------------------------------------------------------------------------------------------------
template <int CINP>
static int lt_launch_forward(const LtFwdArgs& a, int parts, hipStream_t st, const char* what) {
    const size_t lds_bytes = (size_t)(LT_BM + LT_C) * (CINP + 4) * sizeof(float);
    const int rc = ensure_dynamic_lds(reinterpret_cast<const void*>(&lt_forward_kernel<CINP>), lds_bytes, what);
    if (rc != PDSC_OK) return rc;
    hipLaunchKernelGGL((lt_forward_kernel<CINP>), dim3(lt_tiles(a.M), parts), dim3(256), lds_bytes, st, a);
    return check_launch(what);
}

template <int CIS, int PARTS>
static int lt_launch_dx(const LtBwdArgs& a, hipStream_t st, const char* what) {
    const size_t lds_bytes = ((size_t)LT_BM * LT_LDO + (size_t)LT_C * (CIS + 4)) * sizeof(float);
    const int rc = ensure_dynamic_lds(reinterpret_cast<const void*>(&lt_dx_kernel<CIS, PARTS>), lds_bytes, what);
    if (rc != PDSC_OK) return rc;
    hipLaunchKernelGGL((lt_dx_kernel<CIS, PARTS>), dim3(lt_groups(a.M)), dim3(256), lds_bytes, st, a);
    return check_launch(what);
}

template <int CIS>
static int lt_launch_dw(const LtBwdArgs& a, int parts, hipStream_t st, const char* what) {
    const size_t lds_bytes = ((size_t)LT_BM * LT_LDO + (size_t)LT_BM * (CIS + 4)) * sizeof(float);
    const int rc = ensure_dynamic_lds(reinterpret_cast<const void*>(&lt_dw_kernel<CIS>), lds_bytes, what);
    if (rc != PDSC_OK) return rc;
    hipLaunchKernelGGL((lt_dw_kernel<CIS>), dim3(lt_groups(a.M), parts), dim3(256), lds_bytes, st, a);
    return check_launch(what);
}

static int lt_launch_merge(const float* part, int groups, int total, int sets, const LtMergeSegs& sg, hipStream_t st, const char* what) {
    hipLaunchKernelGGL(lt_merge_kernel, dim3(ceil_div(total, 64), sets), dim3(LT_MERGE_THREADS), 0, st, part, groups, total, sg);
    return check_launch(what);
}

template <bool DX, bool DW>
static int lth_launch_backward(const LthArgs& a, hipStream_t st) {
    const size_t lds_bytes = (size_t)LTH_BWD_FLOATS * sizeof(float);
    const int rc = ensure_dynamic_lds(reinterpret_cast<const void*>(&lth_backward_kernel<DX, DW>), lds_bytes,
                                      "pdsc_head_train_backward(dynamic LDS)");
    if (rc != PDSC_OK) return rc;
    hipLaunchKernelGGL((lth_backward_kernel<DX, DW>), dim3(lt_groups(a.M)), dim3(256), lds_bytes, st, a);
    return check_launch("pdsc_head_train_backward");
}

static size_t lt_part_bytes(int M, int Cin, int parts) { return (size_t)parts * lt_groups(M) * ((size_t)LT_C * Cin + LT_C) * sizeof(float); }

}  // namespace pdsc

#define LT_ALIGNED16(p) (((uintptr_t)(p) & 15) == 0)

// ---- plain linear ----------------------------------------------------------------------------------------------------------------
extern "C" size_t pdsc_linear_train_workspace_bytes(int M, int Cin, int Cout) {
    if (M < 1 || !pdsc::lt_shape_ok(Cin, Cout)) return 0;
    return pdsc::lt_part_bytes(M, Cin, 1);
}

extern "C" int pdsc_linear_train_forward(const float* X, const float* W, const float* b, const float* R, float* Y, int M, int Cin,
                                         int Cout, void* stream) {
    PDSC_REQUIRE(X && W && b && Y, "pdsc_linear_train_forward: null pointer");
    PDSC_REQUIRE(pdsc::lt_shape_ok(Cin, Cout), "pdsc_linear_train_forward: (Cin, Cout) = (%d, %d); supported: (1..16, 128) (64, 128)", Cin,
                 Cout);
    PDSC_REQUIRE(M >= 1, "pdsc_linear_train_forward: M=%d", M);
    PDSC_REQUIRE(LT_ALIGNED16(X) && LT_ALIGNED16(W) && LT_ALIGNED16(R) && LT_ALIGNED16(Y),
                 "pdsc_linear_train_forward: X, W, R, Y must be 16-byte aligned");
    pdsc::LtFwdArgs a{};
    a.X = X; a.W0 = a.W1 = a.W2 = W; a.b0 = a.b1 = a.b2 = b; a.R = R; a.Y = Y; a.scale0 = 1.f; a.M = M; a.Cin = Cin; a.ldy = Cout;
    if (Cin == 64) return pdsc::lt_launch_forward<64>(a, 1, (hipStream_t)stream, "pdsc_linear_train_forward");
    return pdsc::lt_launch_forward<16>(a, 1, (hipStream_t)stream, "pdsc_linear_train_forward");
}

extern "C" int pdsc_linear_train_backward(const float* X, const float* W, const float* dY, float* dX, float* dW, float* db, void* ws,
                                          size_t ws_bytes, int M, int Cin, int Cout, void* stream) {
    PDSC_REQUIRE(X && W && dY && ws, "pdsc_linear_train_backward: null pointer");
    PDSC_REQUIRE(dX || dW || db, "pdsc_linear_train_backward: no gradient asked for");
    PDSC_REQUIRE(pdsc::lt_shape_ok(Cin, Cout), "pdsc_linear_train_backward: (Cin, Cout) = (%d, %d); supported: (1..16, 128) (64, 128)", Cin,
                 Cout);
    PDSC_REQUIRE(M >= 1, "pdsc_linear_train_backward: M=%d", M);
    PDSC_REQUIRE(LT_ALIGNED16(X) && LT_ALIGNED16(W) && LT_ALIGNED16(dY) && LT_ALIGNED16(dX) && LT_ALIGNED16(ws),
                 "pdsc_linear_train_backward: X, W, dY, dX and the workspace must be 16-byte aligned");
    const bool want_dw = dW || db;
    const size_t need = pdsc_linear_train_workspace_bytes(M, Cin, Cout);
    if (ws_bytes < need) {
        pdsc::set_error("pdsc_linear_train_backward: workspace of %zu bytes, needs %zu", ws_bytes, need);
        return PDSC_ERR_WORKSPACE;
    }
    hipStream_t st = (hipStream_t)stream;
    pdsc::LtBwdArgs a{};
    a.dY = dY; a.X = X; a.W0 = a.W1 = a.W2 = W; a.dX = dX; a.part = (float*)ws; a.scale0 = 1.f; a.M = M; a.Cin = Cin; a.ldy = Cout;
    int rc = PDSC_OK;
    if (dX) {
        rc = Cin == 64 ? pdsc::lt_launch_dx<64, 1>(a, st, "pdsc_linear_train_backward(dX)")
                       : pdsc::lt_launch_dx<32, 1>(a, st, "pdsc_linear_train_backward(dX)");
        if (rc != PDSC_OK) return rc;
    }
    if (!want_dw) return rc;
    rc = Cin == 64 ? pdsc::lt_launch_dw<64>(a, 1, st, "pdsc_linear_train_backward(dW)")
                   : pdsc::lt_launch_dw<32>(a, 1, st, "pdsc_linear_train_backward(dW)");
    if (rc != PDSC_OK) return rc;
    pdsc::LtMergeSegs sg{};
    for (int k = 0; k < pdsc::LT_MAX_SEGS; ++k) sg.set[k] = -1;
    sg.set[0] = 0; sg.begin[0] = 0; sg.end[0] = Cout * Cin; sg.out[0] = dW;
    sg.set[1] = 0; sg.begin[1] = Cout * Cin; sg.end[1] = Cout * Cin + Cout; sg.out[1] = db;
    return pdsc::lt_launch_merge(a.part, pdsc::lt_groups(M), Cout * Cin + Cout, 1, sg, st, "pdsc_linear_train_backward(merge)");
}

// ---- q|k|v -----------------------------------------------------------------------------------------------------------------------
extern "C" size_t pdsc_qkv_train_workspace_bytes(int M) {
    if (M < 1) return 0;
    return pdsc::lt_part_bytes(M, pdsc::LT_C, 3);
}

extern "C" int pdsc_qkv_train_forward(const float* X, const float* Wq, const float* bq, const float* Wk, const float* bk, const float* Wv,
                                      const float* bv, float q_scale, float* qkv, int M, void* stream) {
    PDSC_REQUIRE(X && Wq && bq && Wk && bk && Wv && bv && qkv, "pdsc_qkv_train_forward: null pointer");
    PDSC_REQUIRE(M >= 1, "pdsc_qkv_train_forward: M=%d", M);
    PDSC_REQUIRE(LT_ALIGNED16(X) && LT_ALIGNED16(Wq) && LT_ALIGNED16(Wk) && LT_ALIGNED16(Wv) && LT_ALIGNED16(qkv),
                 "pdsc_qkv_train_forward: X, Wq, Wk, Wv, qkv must be 16-byte aligned");
    pdsc::LtFwdArgs a{};
    a.X = X; a.W0 = Wq; a.W1 = Wk; a.W2 = Wv; a.b0 = bq; a.b1 = bk; a.b2 = bv; a.R = nullptr; a.Y = qkv; a.scale0 = q_scale;
    a.M = M; a.Cin = pdsc::LT_C; a.ldy = 3 * pdsc::LT_C;
    return pdsc::lt_launch_forward<128>(a, 3, (hipStream_t)stream, "pdsc_qkv_train_forward");
}

extern "C" int pdsc_qkv_train_backward(const float* X, const float* Wq, const float* Wk, const float* Wv, float q_scale, const float* dqkv,
                                       float* dX, float* dWq, float* dbq, float* dWk, float* dbk, float* dWv, float* dbv, void* ws,
                                       size_t ws_bytes, int M, void* stream) {
    PDSC_REQUIRE(X && Wq && Wk && Wv && dqkv && ws, "pdsc_qkv_train_backward: null pointer");
    const bool want_dw = dWq || dbq || dWk || dbk || dWv || dbv;
    PDSC_REQUIRE(dX || want_dw, "pdsc_qkv_train_backward: no gradient asked for");
    PDSC_REQUIRE(M >= 1, "pdsc_qkv_train_backward: M=%d", M);
    PDSC_REQUIRE(LT_ALIGNED16(X) && LT_ALIGNED16(Wq) && LT_ALIGNED16(Wk) && LT_ALIGNED16(Wv) && LT_ALIGNED16(dqkv) && LT_ALIGNED16(dX) &&
                     LT_ALIGNED16(ws),
                 "pdsc_qkv_train_backward: X, Wq, Wk, Wv, dqkv, dX and the workspace must be 16-byte aligned");
    const size_t need = pdsc_qkv_train_workspace_bytes(M);
    if (ws_bytes < need) {
        pdsc::set_error("pdsc_qkv_train_backward: workspace of %zu bytes, needs %zu", ws_bytes, need);
        return PDSC_ERR_WORKSPACE;
    }
    hipStream_t st = (hipStream_t)stream;
    constexpr int C = pdsc::LT_C;
    pdsc::LtBwdArgs a{};
    a.dY = dqkv; a.X = X; a.W0 = Wq; a.W1 = Wk; a.W2 = Wv; a.dX = dX; a.part = (float*)ws; a.scale0 = q_scale; a.M = M; a.Cin = C;
    a.ldy = 3 * C;
    int rc = PDSC_OK;
    if (dX) {
        rc = pdsc::lt_launch_dx<128, 3>(a, st, "pdsc_qkv_train_backward(dX)");
        if (rc != PDSC_OK) return rc;
    }
    if (!want_dw) return rc;
    rc = pdsc::lt_launch_dw<128>(a, 3, st, "pdsc_qkv_train_backward(dW)");
    if (rc != PDSC_OK) return rc;
    pdsc::LtMergeSegs sg{};
    float* dWs[3] = {dWq, dWk, dWv};
    float* dbs[3] = {dbq, dbk, dbv};
    for (int p = 0; p < 3; ++p) {
        sg.set[2 * p] = p; sg.begin[2 * p] = 0; sg.end[2 * p] = C * C; sg.out[2 * p] = dWs[p];
        sg.set[2 * p + 1] = p; sg.begin[2 * p + 1] = C * C; sg.end[2 * p + 1] = C * C + C; sg.out[2 * p + 1] = dbs[p];
    }
    return pdsc::lt_launch_merge(a.part, pdsc::lt_groups(M), C * C + C, 3, sg, st, "pdsc_qkv_train_backward(merge)");
}

// ---- classification head ----------------------------------------------------------------------------------------------------------
extern "C" size_t pdsc_head_train_workspace_bytes(int M) {
    if (M < 1) return 0;
    return (size_t)pdsc::lt_groups(M) * pdsc::LTH_PART * sizeof(float);
}

extern "C" int pdsc_head_train_forward(const float* X, const float* W0, const float* b0, const float* W1, const float* b1, const float* W2,
                                       const float* b2, float* logits, float* pre, int M, void* stream) {
    PDSC_REQUIRE(X && W0 && b0 && W1 && b1 && W2 && b2 && logits, "pdsc_head_train_forward: null pointer");
    PDSC_REQUIRE(M >= 1, "pdsc_head_train_forward: M=%d", M);
    PDSC_REQUIRE(LT_ALIGNED16(X) && LT_ALIGNED16(W0), "pdsc_head_train_forward: X, W0 must be 16-byte aligned");
    const size_t lds_bytes = (size_t)pdsc::LTH_FWD_FLOATS * sizeof(float);
    const int rc = pdsc::ensure_dynamic_lds(reinterpret_cast<const void*>(&pdsc::lth_forward_kernel), lds_bytes,
                                            "pdsc_head_train_forward(dynamic LDS)");
    if (rc != PDSC_OK) return rc;
    pdsc::LthArgs a{};
    a.X = X; a.W0 = W0; a.b0 = b0; a.W1 = W1; a.b1 = b1; a.W2 = W2; a.b2 = b2; a.logits = logits; a.pre = pre; a.M = M;
    hipLaunchKernelGGL(pdsc::lth_forward_kernel, dim3(pdsc::lt_tiles(M)), dim3(256), lds_bytes, (hipStream_t)stream, a);
    return pdsc::check_launch("pdsc_head_train_forward");
}

extern "C" int pdsc_head_train_backward(const float* X, const float* W0, const float* b0, const float* W1, const float* b1, const float* W2,
                                        const float* dlogits, float* dX, float* dW0, float* db0, float* dW1, float* db1, float* dW2,
                                        float* db2, void* ws, size_t ws_bytes, int M, void* stream) {
    PDSC_REQUIRE(X && W0 && b0 && W1 && b1 && W2 && dlogits && ws, "pdsc_head_train_backward: null pointer");
    const bool want_dw = dW0 || db0 || dW1 || db1 || dW2 || db2;
    PDSC_REQUIRE(dX || want_dw, "pdsc_head_train_backward: no gradient asked for");
    PDSC_REQUIRE(M >= 1, "pdsc_head_train_backward: M=%d", M);
    PDSC_REQUIRE(LT_ALIGNED16(X) && LT_ALIGNED16(W0) && LT_ALIGNED16(dX) && LT_ALIGNED16(ws),
                 "pdsc_head_train_backward: X, W0, dX and the workspace must be 16-byte aligned");
    const size_t need = pdsc_head_train_workspace_bytes(M);
    if (ws_bytes < need) {
        pdsc::set_error("pdsc_head_train_backward: workspace of %zu bytes, needs %zu", ws_bytes, need);
        return PDSC_ERR_WORKSPACE;
    }
    hipStream_t st = (hipStream_t)stream;
    pdsc::LthArgs a{};
    a.X = X; a.W0 = W0; a.b0 = b0; a.W1 = W1; a.b1 = b1; a.W2 = W2; a.dL = dlogits; a.dX = dX; a.part = (float*)ws; a.M = M;
    int rc;
    if (dX && want_dw) rc = pdsc::lth_launch_backward<true, true>(a, st);
    else if (dX) rc = pdsc::lth_launch_backward<true, false>(a, st);
    else rc = pdsc::lth_launch_backward<false, true>(a, st);
    if (rc != PDSC_OK || !want_dw) return rc;
    using namespace pdsc;
    LtMergeSegs sg{};
    const int begin[6] = {0, LTH_O_DB0, LTH_O_DW1, LTH_O_DB1, LTH_O_DW2, LTH_O_DB2};
    float* outs[6] = {dW0, db0, dW1, db1, dW2, db2};
    for (int k = 0; k < 6; ++k) {
        sg.set[k] = 0; sg.begin[k] = begin[k]; sg.end[k] = k < 5 ? begin[k + 1] : LTH_PART; sg.out[k] = outs[k];
    }
    return lt_launch_merge(a.part, lt_groups(M), LTH_PART, 1, sg, st, "pdsc_head_train_backward(merge)");
}
