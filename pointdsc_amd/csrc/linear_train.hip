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
// Tiles, products, staging, partials and their merge are train_tile.h's.  dX and dW come from two independent kernels (lt_dx_kernel,
// lt_dw_kernel), so an output that is not wanted costs nothing and the others keep their bits.
#include "train_tile.h"

namespace pdsc {

constexpr int LT_C = 128;                  // output channels of every linear here (per part of q|k|v)
constexpr int LT_LDO = LT_C + TT_PAD;

static bool lt_shape_ok(int Cin, int Cout) { return Cout == LT_C && ((Cin >= 1 && Cin <= 16) || Cin == 64); }

// ---- forward: one workgroup per (64-row tile, part): Y[:, part 128 ..] = (X W_part^T + b_part) s_part (+ R) ------------------
struct LtFwdArgs {
    const float* X; const float* W0; const float* W1; const float* W2; const float* b0; const float* b1; const float* b2;
    const float* R; float* Y;
    float scale0;                // of part 0; the other parts are not scaled
    int M, Cin, ldy;
};

// CINP: K as staged (Cin padded with zeros)
template <int CINP>
__global__ __launch_bounds__(256) void lt_forward_kernel(LtFwdArgs a) {
    constexpr int KP = CINP + TT_PAD, NT = LT_C / 64;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float* Xs = lds;                       // [64][KP]
    float* Ws = lds + TT_BM * KP;          // [128][KP]
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int part = blockIdx.y;
    const int m0 = blockIdx.x * TT_BM;
    const int nrows = min(TT_BM, a.M - m0);
    const float* W = part == 0 ? a.W0 : (part == 1 ? a.W1 : a.W2);
    const float* b = part == 0 ? a.b0 : (part == 1 ? a.b1 : a.b2);
    const float sc = part == 0 ? a.scale0 : 1.f;

    tt_stage_rows<CINP>(a.X, m0, Xs, TT_BM, nrows, a.Cin);
    tt_stage_rows<CINP>(W, 0, Ws, LT_C, LT_C, a.Cin);
    __syncthreads();

    const int wm = wave & 1, wn = wave >> 1;
    const int l31 = lane & 31, h = lane >> 5;
    f32x16 acc[NT];
    tt_zero(acc);
    tt_mma_rows_rows<CINP, NT, 2>(Xs + wm * 32 * KP, KP, Ws + wn * NT * 32 * KP, KP, acc);

#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        const int n = (wn * NT + nt) * 32 + l31;
        const float bval = b[n];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int i = wm * 32 + tt_acc_row(r, h);
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
    for (int i = 0; i < TT_BM / 8; ++i) {
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

// ---- backward, dX: persistent workgroups walk the tiles; dX tile = sum over the parts of dY_p W_p --------------------------
// CIS: Cin as staged (32 for Cin <= 16: the matrix instruction's N is 32; 64; 128).  PARTS == 1: W staged once per workgroup.
template <int CIS, int PARTS>
__global__ __launch_bounds__(256) void lt_dx_kernel(LtBwdArgs a) {
    constexpr int LDI = CIS + TT_PAD;
    constexpr int NTI = CIS >= 64 ? CIS / 64 : 1;            // 32-column blocks per wave
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float* dYs = lds;                                        // [64][LT_LDO]
    float* Ws = dYs + TT_BM * LT_LDO;                        // [128][LDI]
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, l31 = lane & 31, h = lane >> 5;
    const int wm = wave & 1, wn = wave >> 1;
    const bool active = wn * NTI * 32 < CIS;                 // CIS == 32: two of the four waves own the 64 x 32 tile
    const int tiles = ceil_div_dev(a.M, TT_BM);
    float unused[4] = {0.f, 0.f, 0.f, 0.f};

    if (PARTS == 1) tt_stage_rows<CIS>(a.W0, 0, Ws, LT_C, LT_C, a.Cin);
    for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int m0 = tile * TT_BM;
        const int nrows = min(TT_BM, a.M - m0);
        f32x16 acc[NTI];
        tt_zero(acc);
#pragma unroll 1
        for (int p = 0; p < PARTS; ++p) {
            __syncthreads();                                 // the previous readers are done
            lt_stage_dy<false>(a, dYs, m0, nrows, p, unused);
            if (PARTS > 1) tt_stage_rows<CIS>(p == 0 ? a.W0 : (p == 1 ? a.W1 : a.W2), 0, Ws, LT_C, LT_C, a.Cin);
            __syncthreads();
            // dX[m][ci] += sum_co dY[m][co] W[co][ci]
            if (active) tt_mma_rows_cols<LT_C, NTI, 2>(dYs + wm * 32 * LT_LDO, LT_LDO, Ws + wn * NTI * 32, LDI, acc);
        }
        if (active) {
#pragma unroll
            for (int nt = 0; nt < NTI; ++nt) {
                const int n = (wn * NTI + nt) * 32 + l31;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int i = wm * 32 + tt_acc_row(r, h);
                    if (i < nrows && n < a.Cin) a.dX[(size_t)(m0 + i) * a.Cin + n] = acc[nt][r];
                }
            }
        }
    }
}

// ---- backward, dW and db: workgroup (g, p) walks the tiles g, g + groups, ... of part p: dW_p += dY_p^T X, db_p += sum dY_p ---
template <int CIS>
__global__ __launch_bounds__(256) void lt_dw_kernel(LtBwdArgs a) {
    constexpr int LDI = CIS + TT_PAD;
    constexpr int CIB = CIS / 32, TPW = CIB;                 // 32 x 32 blocks of dW: 4 x CIB, TPW per wave
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float* dYs = lds;                                        // [64][LT_LDO]
    float* Xs = dYs + TT_BM * LT_LDO;                        // [64][LDI]
    const int t = threadIdx.x, wave = t >> 6;
    const int p = blockIdx.y;
    const int tiles = ceil_div_dev(a.M, TT_BM);
    float dbs[4] = {0.f, 0.f, 0.f, 0.f};
    f32x16 accw[TPW];
    tt_zero(accw);

    for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int m0 = tile * TT_BM;
        const int nrows = min(TT_BM, a.M - m0);
        __syncthreads();
        lt_stage_dy<true>(a, dYs, m0, nrows, p, dbs);
        tt_stage_rows<CIS>(a.X, m0, Xs, TT_BM, nrows, a.Cin);
        __syncthreads();
        // dW[co][ci] += sum_rows dY[row][co] X[row][ci]: block (co, ci) = (j / CIB, j % CIB)
        tt_mma_cols_cols<TT_BM, TPW, CIB, 4>(dYs, LT_LDO, Xs, LDI, wave * TPW, accw);
    }

    float* P = a.part + ((size_t)p * gridDim.x + blockIdx.x) * (LT_C * a.Cin + LT_C);
    tt_write_dw_blocks<TPW, CIB>(P, a.Cin, a.Cin, wave * TPW, accw);
    const float s = tt_column_sums<8, LT_C>(dYs, dbs, t >> 5, (t & 31) * 4, 1);      // db; the dY tile has no readers left
    if (t < LT_C) P[LT_C * a.Cin + t] = s;
}

// ---- the classification head ---------------------------------------------------------------------------------------------------
constexpr int LTH_CIN = 128, LTH_H = 32;
constexpr int LTH_LDX = LTH_CIN + TT_PAD;  // X tile and W0 rows
constexpr int LTH_LDH = LTH_H + TT_PAD;       // W1 rows, A0, dA0, dA1 (16-byte reads along a row)
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
constexpr int LTH_FWD_FLOATS = TT_BM * LTH_LDX + LTH_H * LTH_LDX + LTH_H * LTH_LDH + TT_BM * LTH_LDH + TT_BM * LTH_LDA + 3 * LTH_H;

__device__ __forceinline__ LthLds lth_carve(float* lds) {
    LthLds s;
    s.Xs = lds;
    s.W0s = s.Xs + TT_BM * LTH_LDX;
    s.W1s = s.W0s + LTH_H * LTH_LDX;
    s.A0s = s.W1s + LTH_H * LTH_LDH;
    s.A1s = s.A0s + TT_BM * LTH_LDH;
    s.b0s = s.A1s + TT_BM * LTH_LDA;
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
    tt_stage_rows16<LTH_CIN>(a.W0, 0, s.W0s, LTH_H, LTH_H);
    tt_stage_rows_scalar<LTH_H>(a.W1, 0, s.W1s, LTH_H, LTH_H, LTH_H);
    if (t < LTH_H) { s.b0s[t] = a.b0[t]; s.b1s[t] = a.b1[t]; s.w2s[t] = a.W2[t]; }
}

// A0 = X W0^T + b0, A1 = relu(A0) W1^T + b1 of the staged tile; the forward and the backward both call THIS, so the backward's
// masks A0 > 0, A1 > 0 are the forward's bits.  Waves 0 and 1 own 32 rows each (a 32 x 32 output block); ends with a barrier.
__device__ __forceinline__ void lth_hidden(const LthLds& s) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l31 = lane & 31, h = lane >> 5;
    __syncthreads();                                         // the stage is complete
    if (wave < 2) {
        f32x16 acc[1];
        tt_zero(acc);
        tt_mma_rows_rows<LTH_CIN, 1, 4>(s.Xs + wave * 32 * LTH_LDX, LTH_LDX, s.W0s, LTH_LDX, acc);
        const float bval = s.b0s[l31];
#pragma unroll
        for (int r = 0; r < 16; ++r) s.A0s[(wave * 32 + tt_acc_row(r, h)) * LTH_LDH + l31] = acc[0][r] + bval;
    }
    __syncthreads();
    if (wave < 2) {
        f32x16 acc[1];
        tt_zero(acc);
        tt_mma_rows_rows<LTH_H, 1, 4, true>(s.A0s + wave * 32 * LTH_LDH, LTH_LDH, s.W1s, LTH_LDH, acc);      // relu(A0) as it is read
        const float bval = s.b1s[l31];
#pragma unroll
        for (int r = 0; r < 16; ++r) s.A1s[(wave * 32 + tt_acc_row(r, h)) * LTH_LDA + l31] = acc[0][r] + bval;
    }
    __syncthreads();
}

__global__ __launch_bounds__(256) void lth_forward_kernel(LthArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const LthLds s = lth_carve(lds);
    const int t = threadIdx.x;
    const int m0 = blockIdx.x * TT_BM;
    const int nrows = min(TT_BM, a.M - m0);
    lth_stage_weights(a, s);
    tt_stage_rows16<LTH_CIN>(a.X, m0, s.Xs, TT_BM, nrows);
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
    float* G1s = G0s + TT_BM * LTH_LDH;                      // dA1 [64][LTH_LDH]
    float* dLs = G1s + TT_BM * LTH_LDH;                      // [64]
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, l31 = lane & 31, h = lane >> 5;
    const int j = t & 31, rl = t >> 5;                       // element-wise passes: thread = column j of rows rl, rl + 8, ...
    const int tiles = ceil_div_dev(a.M, TT_BM);
    float sums[4] = {0.f, 0.f, 0.f, 0.f};                    // of column j: db0, db1, dW2, db2 (the last the same in every column)
    f32x16 accw0[1], accw1[1];
    tt_zero(accw0);
    tt_zero(accw1);

    lth_stage_weights(a, s);
    for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int m0 = tile * TT_BM;
        const int nrows = min(TT_BM, a.M - m0);
        __syncthreads();                                     // the previous tile's readers are done
        tt_stage_rows16<LTH_CIN>(a.X, m0, s.Xs, TT_BM, nrows);
        if (t < TT_BM) dLs[t] = t < nrows ? a.dL[m0 + t] : 0.f;
        lth_hidden(s);

        const float w2 = s.w2s[j];
#pragma unroll
        for (int i = 0; i < TT_BM / 8; ++i) {
            const int r = rl + 8 * i;
            const float a1 = s.A1s[r * LTH_LDA + j], dl = dLs[r];
            const float g = a1 > 0.f ? dl * w2 : 0.f;
            G1s[r * LTH_LDH + j] = g;
            sums[1] += g;
            sums[2] = fmaf(dl, fmaxf(a1, 0.f), sums[2]);
            sums[3] += dl;
        }
        __syncthreads();
        if (wave < 2) {
            // dH0[m][j0] = sum_j1 dA1[m][j1] W1[j1][j0]
            f32x16 acc[1];
            tt_zero(acc);
            tt_mma_rows_cols<LTH_H, 1, 4>(G1s + wave * 32 * LTH_LDH, LTH_LDH, s.W1s, LTH_LDH, acc);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int i = wave * 32 + tt_acc_row(r, h);
                G0s[i * LTH_LDH + l31] = s.A0s[i * LTH_LDH + l31] > 0.f ? acc[0][r] : 0.f;
            }
        }
        __syncthreads();

        if (DX) {
            // dX[m][ci] = sum_j0 dA0[m][j0] W0[j0][ci]
            const int wm = wave & 1, wn = wave >> 1;
            f32x16 acc[2];
            tt_zero(acc);
            tt_mma_rows_cols<LTH_H, 2, 4>(G0s + wm * 32 * LTH_LDH, LTH_LDH, s.W0s + wn * 64, LTH_LDX, acc);
#pragma unroll
            for (int nt = 0; nt < 2; ++nt) {
                const int n = wn * 64 + nt * 32 + l31;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int i = wm * 32 + tt_acc_row(r, h);
                    if (i < nrows) a.dX[(size_t)(m0 + i) * LTH_CIN + n] = acc[nt][r];
                }
            }
        }
        if (DW) {
#pragma unroll
            for (int i = 0; i < TT_BM / 8; ++i) sums[0] += G0s[(rl + 8 * i) * LTH_LDH + j];
            // dW0[j0][ci] += sum_rows dA0[row][j0] X[row][ci]: wave = 32-column block of ci
            tt_mma_cols_cols<TT_BM, 1, LTH_CIN / 32, 4>(G0s, LTH_LDH, s.Xs, LTH_LDX, wave, accw0);
            // dW1[j1][j0] += sum_rows dA1[row][j1] relu(A0[row][j0]): one block, wave 3 (rows past the end: dA1 = 0)
            if (wave == 3) tt_mma_cols_cols<TT_BM, 1, 1, 4, true>(G1s, LTH_LDH, s.A0s, LTH_LDH, 0, accw1);
        }
    }

    if (DW) {
        float* P = a.part + (size_t)blockIdx.x * LTH_PART;
        tt_write_dw_blocks<1, LTH_CIN / 32>(P, LTH_CIN, LTH_CIN, wave, accw0);
        if (wave == 3) tt_write_dw_blocks<1, 1>(P + LTH_O_DW1, LTH_H, LTH_H, 0, accw1);
        // the element-wise sums: thread t < 128 = (which, j); the dA0 tile has no readers left
        const float v = tt_column_sums<8, 4 * LTH_H>(G0s, sums, rl, j, LTH_H);
        const int which = t >> 5;
        if (which == 0) P[LTH_O_DB0 + j] = v;
        else if (which == 1) P[LTH_O_DB1 + j] = v;
        else if (which == 2) P[LTH_O_DW2 + j] = v;
        else if (t == 3 * LTH_H) P[LTH_O_DB2] = v;
    }
}
constexpr int LTH_BWD_FLOATS = LTH_FWD_FLOATS + 2 * TT_BM * LTH_LDH + TT_BM;

// ---- launchers -------------------------------------------------------------------------------------------------------------------
template <int CINP>
static int lt_launch_forward(const LtFwdArgs& a, int parts, hipStream_t st, const char* what) {
    return launch_with_dynamic_lds(lt_forward_kernel<CINP>, dim3(tt_tiles(a.M), parts), (size_t)(TT_BM + LT_C) * (CINP + TT_PAD) * sizeof(float),
                                   st, what, a);
}

template <int CIS, int PARTS>
static int lt_launch_dx(const LtBwdArgs& a, hipStream_t st, const char* what) {
    return launch_with_dynamic_lds(lt_dx_kernel<CIS, PARTS>, dim3(tt_groups(a.M)),
                                   ((size_t)TT_BM * LT_LDO + (size_t)LT_C * (CIS + TT_PAD)) * sizeof(float), st, what, a);
}

template <int CIS>
static int lt_launch_dw(const LtBwdArgs& a, int parts, hipStream_t st, const char* what) {
    return launch_with_dynamic_lds(lt_dw_kernel<CIS>, dim3(tt_groups(a.M), parts),
                                   ((size_t)TT_BM * LT_LDO + (size_t)TT_BM * (CIS + TT_PAD)) * sizeof(float), st, what, a);
}

template <bool DX, bool DW>
static int lth_launch_backward(const LthArgs& a, hipStream_t st) {
    return launch_with_dynamic_lds(lth_backward_kernel<DX, DW>, dim3(tt_groups(a.M)), (size_t)LTH_BWD_FLOATS * sizeof(float), st,
                                   "pdsc_head_train_backward", a);
}

static size_t lt_part_bytes(int M, int Cin, int parts) { return (size_t)parts * tt_groups(M) * ((size_t)LT_C * Cin + LT_C) * sizeof(float); }

}  // namespace pdsc

using pdsc::aligned16;

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
    PDSC_REQUIRE(aligned16(X) && aligned16(W) && aligned16(R) && aligned16(Y),
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
    PDSC_REQUIRE(aligned16(X) && aligned16(W) && aligned16(dY) && aligned16(dX) && aligned16(ws),
                 "pdsc_linear_train_backward: X, W, dY, dX and the workspace must be 16-byte aligned");
    const bool want_dw = dW || db;
    int rc = pdsc::check_workspace("pdsc_linear_train_backward", ws_bytes, pdsc_linear_train_workspace_bytes(M, Cin, Cout));
    if (rc != PDSC_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    pdsc::LtBwdArgs a{};
    a.dY = dY; a.X = X; a.W0 = a.W1 = a.W2 = W; a.dX = dX; a.part = (float*)ws; a.scale0 = 1.f; a.M = M; a.Cin = Cin; a.ldy = Cout;
    if (dX) {
        rc = Cin == 64 ? pdsc::lt_launch_dx<64, 1>(a, st, "pdsc_linear_train_backward(dX)")
                       : pdsc::lt_launch_dx<32, 1>(a, st, "pdsc_linear_train_backward(dX)");
        if (rc != PDSC_OK) return rc;
    }
    if (!want_dw) return rc;
    rc = Cin == 64 ? pdsc::lt_launch_dw<64>(a, 1, st, "pdsc_linear_train_backward(dW)")
                   : pdsc::lt_launch_dw<32>(a, 1, st, "pdsc_linear_train_backward(dW)");
    if (rc != PDSC_OK) return rc;
    pdsc::TtMergeSegs sg{};
    sg.add(0, 0, Cout * Cin, dW);
    sg.add(0, Cout * Cin, Cout * Cin + Cout, db);
    return pdsc::tt_launch_merge(a.part, pdsc::tt_groups(M), Cout * Cin + Cout, 1, sg, st, "pdsc_linear_train_backward(merge)");
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
    PDSC_REQUIRE(aligned16(X) && aligned16(Wq) && aligned16(Wk) && aligned16(Wv) && aligned16(qkv),
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
    PDSC_REQUIRE(aligned16(X) && aligned16(Wq) && aligned16(Wk) && aligned16(Wv) && aligned16(dqkv) && aligned16(dX) &&
                     aligned16(ws),
                 "pdsc_qkv_train_backward: X, Wq, Wk, Wv, dqkv, dX and the workspace must be 16-byte aligned");
    int rc = pdsc::check_workspace("pdsc_qkv_train_backward", ws_bytes, pdsc_qkv_train_workspace_bytes(M));
    if (rc != PDSC_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    constexpr int C = pdsc::LT_C;
    pdsc::LtBwdArgs a{};
    a.dY = dqkv; a.X = X; a.W0 = Wq; a.W1 = Wk; a.W2 = Wv; a.dX = dX; a.part = (float*)ws; a.scale0 = q_scale; a.M = M; a.Cin = C;
    a.ldy = 3 * C;
    if (dX) {
        rc = pdsc::lt_launch_dx<128, 3>(a, st, "pdsc_qkv_train_backward(dX)");
        if (rc != PDSC_OK) return rc;
    }
    if (!want_dw) return rc;
    rc = pdsc::lt_launch_dw<128>(a, 3, st, "pdsc_qkv_train_backward(dW)");
    if (rc != PDSC_OK) return rc;
    pdsc::TtMergeSegs sg{};
    float* dWs[3] = {dWq, dWk, dWv};
    float* dbs[3] = {dbq, dbk, dbv};
    for (int p = 0; p < 3; ++p) {
        sg.add(p, 0, C * C, dWs[p]);
        sg.add(p, C * C, C * C + C, dbs[p]);
    }
    return pdsc::tt_launch_merge(a.part, pdsc::tt_groups(M), C * C + C, 3, sg, st, "pdsc_qkv_train_backward(merge)");
}

// ---- classification head ----------------------------------------------------------------------------------------------------------
extern "C" size_t pdsc_head_train_workspace_bytes(int M) {
    if (M < 1) return 0;
    return (size_t)pdsc::tt_groups(M) * pdsc::LTH_PART * sizeof(float);
}

extern "C" int pdsc_head_train_forward(const float* X, const float* W0, const float* b0, const float* W1, const float* b1, const float* W2,
                                       const float* b2, float* logits, float* pre, int M, void* stream) {
    PDSC_REQUIRE(X && W0 && b0 && W1 && b1 && W2 && b2 && logits, "pdsc_head_train_forward: null pointer");
    PDSC_REQUIRE(M >= 1, "pdsc_head_train_forward: M=%d", M);
    PDSC_REQUIRE(aligned16(X) && aligned16(W0), "pdsc_head_train_forward: X, W0 must be 16-byte aligned");
    pdsc::LthArgs a{};
    a.X = X; a.W0 = W0; a.b0 = b0; a.W1 = W1; a.b1 = b1; a.W2 = W2; a.b2 = b2; a.logits = logits; a.pre = pre; a.M = M;
    return pdsc::launch_with_dynamic_lds(pdsc::lth_forward_kernel, dim3(pdsc::tt_tiles(M)), (size_t)pdsc::LTH_FWD_FLOATS * sizeof(float),
                                         (hipStream_t)stream, "pdsc_head_train_forward", a);
}

extern "C" int pdsc_head_train_backward(const float* X, const float* W0, const float* b0, const float* W1, const float* b1, const float* W2,
                                        const float* dlogits, float* dX, float* dW0, float* db0, float* dW1, float* db1, float* dW2,
                                        float* db2, void* ws, size_t ws_bytes, int M, void* stream) {
    PDSC_REQUIRE(X && W0 && b0 && W1 && b1 && W2 && dlogits && ws, "pdsc_head_train_backward: null pointer");
    const bool want_dw = dW0 || db0 || dW1 || db1 || dW2 || db2;
    PDSC_REQUIRE(dX || want_dw, "pdsc_head_train_backward: no gradient asked for");
    PDSC_REQUIRE(M >= 1, "pdsc_head_train_backward: M=%d", M);
    PDSC_REQUIRE(aligned16(X) && aligned16(W0) && aligned16(dX) && aligned16(ws),
                 "pdsc_head_train_backward: X, W0, dX and the workspace must be 16-byte aligned");
    int rc = pdsc::check_workspace("pdsc_head_train_backward", ws_bytes, pdsc_head_train_workspace_bytes(M));
    if (rc != PDSC_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    pdsc::LthArgs a{};
    a.X = X; a.W0 = W0; a.b0 = b0; a.W1 = W1; a.b1 = b1; a.W2 = W2; a.dL = dlogits; a.dX = dX; a.part = (float*)ws; a.M = M;
    if (dX && want_dw) rc = pdsc::lth_launch_backward<true, true>(a, st);
    else if (dX) rc = pdsc::lth_launch_backward<true, false>(a, st);
    else rc = pdsc::lth_launch_backward<false, true>(a, st);
    if (rc != PDSC_OK || !want_dw) return rc;
    using namespace pdsc;
    TtMergeSegs sg{};
    const int begin[7] = {0, LTH_O_DB0, LTH_O_DW1, LTH_O_DB1, LTH_O_DW2, LTH_O_DB2, LTH_PART};
    float* outs[6] = {dW0, db0, dW1, db1, dW2, db2};
    for (int k = 0; k < 6; ++k) sg.add(0, begin[k], begin[k + 1], outs[k]);
    return tt_launch_merge(a.part, tt_groups(M), LTH_PART, 1, sg, st, "pdsc_head_train_backward(merge)");
}
