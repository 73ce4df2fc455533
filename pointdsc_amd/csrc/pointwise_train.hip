// f-15: the encoder's point-wise layers in train() mode, Conv1d(k=1) -> BatchNorm1d (batch statistics) -> ReLU, forward and
// backward on channel-last rows (reference: models/PointDSC.py:12-23,54-61 under model.train()).
//
//   forward   Y = X W^T + b;  mean, var (biased) per channel over the M rows;  invstd = 1 / sqrt(var + eps);
//             Z = relu(gamma (Y - mean) invstd + beta);  running statistics as F.batch_norm(training=True) updates them.
//   backward  g = dZ [Z > 0];  dbeta = sum g;  dgamma = sum g xh;  dY = gamma invstd (g - dbeta / M - xh dgamma / M);
//             db = sum dY;  dW = dY^T X;  dX = dY W.
//
// The three products, the staging, the dW / db partials and their merge are train_tile.h's.  Launch sequences:
//   forward   1. pwt_forward_gemm_kernel   one workgroup per 64-row tile: Y, and the tile's (mean, M2) per channel in fp64
//             2. pwt_stats_merge_kernel    16 channels per workgroup: mean = sum n_t mean_t / M, M2 = sum M2_t + n_t (mean_t - mean)^2 in fp64
//                                          (mean-centred throughout: no E[y^2] - E[y]^2), invstd, running statistics in place
//             3. pwt_norm_relu_kernel      Z
//   backward  1. pwt_backward_reduce_kernel  one workgroup per tile: fp64 partials of dbeta, dgamma
//             2. pwt_sum_partials_kernel     16 columns per workgroup: the tiles' partials in a fixed order
//             3. pwt_backward_gemm_kernel    persistent workgroups (at most one per compute unit) walk the tiles: dY rebuilt per
//                                            tile in LDS, dX tile written, dW accumulated in registers over the workgroup's tiles;
//                                            one [Cout][Cin] (+ db [Cout]) partial per workgroup
//             4. tt_merge_kernel             the workgroups' partials in index order -> dW, db
// The ReLU mask of the backward is recomputed from Y with the forward's own expression (pwt_preact): the same bits as Z > 0,
// and Z is not read again.
#include "train_tile.h"

namespace pdsc {

constexpr int PWT_MERGE_THREADS = TT_MERGE_THREADS;
constexpr int PWT_MERGE_COLS = 16;         // channels per workgroup of the two statistics merges (64 slices of tiles each)

__device__ __forceinline__ float pwt_xhat(float y, float mean, float invstd) { return (y - mean) * invstd; }
__device__ __forceinline__ float pwt_preact(float xh, float gamma, float beta) { return fmaf(gamma, xh, beta); }
// the backward's arithmetic behind the mask runs in fp64 (a few operations per element, beside a 128-deep product): with few rows
// dY is a small difference of O(1) terms, and fp32 roundings of xh, mean or invstd would be most of it.  So mean and invstd travel
// from the forward to the backward in fp64; the forward's Z and the backward's mask use their fp32 roundings, both alike.
__device__ __forceinline__ double pwt_xhat_f64(float y, double mean, double invstd) { return ((double)y - mean) * invstd; }

static bool pwt_shape_ok(int Cin, int Cout) { return (Cin == 128 && (Cout == 128 || Cout == 64)) || (Cin == 64 && Cout == 64); }

// workspace: [tiles][2][Cout] fp64 (forward: mean_t, M2_t; backward: dbeta_t, dgamma_t) | [2][Cout] fp64 (dbeta / M, dgamma / M) |
//            [groups][Cout * Cin + Cout] fp32 (dW, db partials)
static size_t pwt_part_bytes(int M, int Cout) { return (size_t)tt_tiles(M) * 2 * Cout * sizeof(double); }
static size_t pwt_sums_bytes(int Cout) { return (size_t)2 * Cout * sizeof(double); }
static size_t pwt_dw_bytes(int M, int Cin, int Cout) { return (size_t)tt_groups(M) * ((size_t)Cout * Cin + Cout) * sizeof(float); }

struct PwtFwdArgs {
    const float* X; const float* W; const float* b;
    float* Y; double* part;
    int M;
};

// ---- forward 1: Y tile on the matrix cores, the tile's mean and M2 per channel -------------------------------------------
template <int CIN, int COUT>
__global__ __launch_bounds__(256) void pwt_forward_gemm_kernel(PwtFwdArgs a) {
    constexpr int KP = CIN + TT_PAD, NT = COUT / 64, LDY = COUT + 1;
    static_assert(LDY <= KP, "the Y tile reuses the X stage");
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float* Xs = lds;                       // [64][KP], then the Y tile [64][LDY]
    float* Ws = lds + TT_BM * KP;         // [COUT][KP]
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int m0 = blockIdx.x * TT_BM;
    const int nrows = min(TT_BM, a.M - m0);

    tt_stage_rows16<CIN>(a.X, m0, Xs, TT_BM, nrows);
    tt_stage_rows16<CIN>(a.W, 0, Ws, COUT, COUT);
    __syncthreads();

    const int wm = wave & 1, wn = wave >> 1;
    const int l31 = lane & 31, h = lane >> 5;
    f32x16 acc[NT];
    tt_zero(acc);
    tt_mma_rows_rows<CIN, NT, 4>(Xs + wm * 32 * KP, KP, Ws + wn * NT * 32 * KP, KP, acc);
    __syncthreads();                       // every wave has read its X rows: the stage becomes the Y tile

    float* Ys = Xs;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        const int n = (wn * NT + nt) * 32 + l31;
        const float bval = a.b[n];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int i = wm * 32 + tt_acc_row(r, h);
            const float v = acc[nt][r] + bval;
            Ys[i * LDY + n] = v;
            if (i < nrows) a.Y[(size_t)(m0 + i) * COUT + n] = v;
        }
    }
    __syncthreads();

    // mean-centred tile statistics in fp64, rows in order: thread = channel
    if (t < COUT) {
        double s = 0.0;
        for (int r = 0; r < nrows; ++r) s += (double)Ys[r * LDY + t];
        const double mean = s / (double)nrows;
        double m2 = 0.0;
        for (int r = 0; r < nrows; ++r) {
            const double d = (double)Ys[r * LDY + t] - mean;
            m2 = fma(d, d, m2);
        }
        a.part[((size_t)blockIdx.x * 2 + 0) * COUT + t] = mean;
        a.part[((size_t)blockIdx.x * 2 + 1) * COUT + t] = m2;
    }
}

// ---- forward 2: the tiles' statistics -> mean, invstd, running statistics -------------------------------------------------
// One workgroup per PWT_MERGE_COLS channels; thread = (slice s, channel): a slice adds the tiles s, s + 64, ... in order, then one
// thread per channel adds the 64 slices in order (a thread walks few tiles: the walk is a chain of load latencies).
__global__ __launch_bounds__(PWT_MERGE_THREADS) void pwt_stats_merge_kernel(const double* __restrict__ part, int tiles, int M, int Cout,
                                                                           float momentum, float eps, float* __restrict__ running_mean,
                                                                           float* __restrict__ running_var, double* __restrict__ mean_out,
                                                                           double* __restrict__ invstd_out) {
    __shared__ double red[PWT_MERGE_THREADS];
    constexpr int S = PWT_MERGE_THREADS / PWT_MERGE_COLS;
    const int t = threadIdx.x, cl = t % PWT_MERGE_COLS, s = t / PWT_MERGE_COLS, c = blockIdx.x * PWT_MERGE_COLS + cl;
    double acc = 0.0;
    for (int tile = s; tile < tiles; tile += S) {
        const double n = (double)min(TT_BM, M - tile * TT_BM);
        acc = fma(n, part[((size_t)tile * 2) * Cout + c], acc);
    }
    red[t] = acc;
    __syncthreads();
    double tot = 0.0;
#pragma unroll 16
    for (int j = 0; j < S; ++j) tot += red[j * PWT_MERGE_COLS + cl];
    const double mean = tot / (double)M;
    __syncthreads();
    acc = 0.0;
    for (int tile = s; tile < tiles; tile += S) {
        const double n = (double)min(TT_BM, M - tile * TT_BM);
        const double d = part[((size_t)tile * 2) * Cout + c] - mean;
        acc += part[((size_t)tile * 2 + 1) * Cout + c] + n * d * d;
    }
    red[t] = acc;
    __syncthreads();
    if (s == 0) {
        double m2 = 0.0;
#pragma unroll 16
        for (int j = 0; j < S; ++j) m2 += red[j * PWT_MERGE_COLS + cl];
        const double var = m2 / (double)M;
        mean_out[c] = mean;
        invstd_out[c] = 1.0 / sqrt(var + (double)eps);
        const double mom = (double)momentum;
        running_mean[c] = (float)((1.0 - mom) * (double)running_mean[c] + mom * mean);
        running_var[c] = (float)((1.0 - mom) * (double)running_var[c] + mom * (m2 / (double)(M - 1)));
    }
}

// ---- forward 3: Z = relu(gamma xh + beta); thread = 4 channels of a row ----------------------------------------------------
__global__ __launch_bounds__(256) void pwt_norm_relu_kernel(const float* __restrict__ Y, const double* __restrict__ mean,
                                                            const double* __restrict__ invstd, const float* __restrict__ gamma,
                                                            const float* __restrict__ beta, float* __restrict__ Z, int M, int Cout) {
    const int c4n = Cout >> 2;
    const int c4 = (threadIdx.x % c4n) * 4, rl = threadIdx.x / c4n, RL = 256 / c4n;
    float mu[4], is[4], ga[4], be[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) { mu[e] = (float)mean[c4 + e]; is[e] = (float)invstd[c4 + e]; ga[e] = gamma[c4 + e]; be[e] = beta[c4 + e]; }
    for (long long row = (long long)blockIdx.x * RL + rl; row < M; row += (long long)gridDim.x * RL) {
        const f32x4 y = *reinterpret_cast<const f32x4*>(Y + row * Cout + c4);
        f32x4 z;
#pragma unroll
        for (int e = 0; e < 4; ++e) z[e] = fmaxf(pwt_preact(pwt_xhat(y[e], mu[e], is[e]), ga[e], be[e]), 0.f);
        *reinterpret_cast<f32x4*>(Z + row * Cout + c4) = z;
    }
}

// ---- backward 1: the tile's dbeta, dgamma in fp64 --------------------------------------------------------------------------
template <int COUT>
__global__ __launch_bounds__(256) void pwt_backward_reduce_kernel(const float* __restrict__ Y, const float* __restrict__ dZ,
                                                                  const double* __restrict__ mean, const double* __restrict__ invstd,
                                                                  const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                  double* __restrict__ part, int M) {
    constexpr int C4N = COUT / 4, RL = 256 / C4N;
    __shared__ double red[RL * 2 * COUT];
    const int t = threadIdx.x, c4 = (t % C4N) * 4, rl = t / C4N;
    const int m0 = blockIdx.x * TT_BM;
    const int nrows = min(TT_BM, M - m0);
    float mu[4], is[4], ga[4], be[4];
    double mud[4], isd[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        mud[e] = mean[c4 + e]; isd[e] = invstd[c4 + e]; ga[e] = gamma[c4 + e]; be[e] = beta[c4 + e];
        mu[e] = (float)mud[e]; is[e] = (float)isd[e];
    }
    double sb[4] = {0.0, 0.0, 0.0, 0.0}, sg[4] = {0.0, 0.0, 0.0, 0.0};
    for (int r = rl; r < nrows; r += RL) {
        const f32x4 y = *reinterpret_cast<const f32x4*>(Y + (size_t)(m0 + r) * COUT + c4);
        const f32x4 dz = *reinterpret_cast<const f32x4*>(dZ + (size_t)(m0 + r) * COUT + c4);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float g = pwt_preact(pwt_xhat(y[e], mu[e], is[e]), ga[e], be[e]) > 0.f ? dz[e] : 0.f;      // the forward's mask
            sb[e] += (double)g;
            sg[e] += (double)g * pwt_xhat_f64(y[e], mud[e], isd[e]);
        }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        red[(rl * 2 + 0) * COUT + c4 + e] = sb[e];
        red[(rl * 2 + 1) * COUT + c4 + e] = sg[e];
    }
    __syncthreads();
    if (t < 2 * COUT) {
        double s = 0.0;
#pragma unroll
        for (int j = 0; j < RL; ++j) s += red[j * 2 * COUT + t];
        part[(size_t)blockIdx.x * 2 * COUT + t] = s;
    }
}

// ---- backward 2: partials [tiles][ncol] fp64 in tile order (ncol = 2 Cout: dbeta | dgamma) -> the sums (fp32, to the caller) and
//      the sums / M (fp64; what backward 3 subtracts) -------------------------------------------------------------------------
__global__ __launch_bounds__(PWT_MERGE_THREADS) void pwt_sum_partials_kernel(const double* __restrict__ part, int tiles, int ncol, int M,
                                                                            double* __restrict__ means, float* __restrict__ out0,
                                                                            float* __restrict__ out1) {
    __shared__ double red[PWT_MERGE_THREADS];
    constexpr int S = PWT_MERGE_THREADS / PWT_MERGE_COLS;
    const int t = threadIdx.x, cl = t % PWT_MERGE_COLS, s = t / PWT_MERGE_COLS, c = blockIdx.x * PWT_MERGE_COLS + cl;
    double acc = 0.0;
    for (int tile = s; tile < tiles; tile += S) acc += part[(size_t)tile * ncol + c];
    red[t] = acc;
    __syncthreads();
    if (s == 0) {
        double tot = 0.0;
#pragma unroll 16
        for (int j = 0; j < S; ++j) tot += red[j * PWT_MERGE_COLS + cl];
        const float v = (float)tot;
        means[c] = tot / (double)M;
        const int half = ncol >> 1;
        if (c < half) { if (out0) out0[c] = v; }
        else if (out1) out1[c - half] = v;
    }
}

struct PwtBwdArgs {
    const float* X; const float* W; const float* Y; const float* dZ;
    const double* mean; const double* invstd; const float* gamma; const float* beta;
    const double* means;         // [2][Cout]: dbeta / M, dgamma / M
    float* dX; float* dwpart;    // dwpart [groups][Cout * Cin + Cout]
    int M;
};

// ---- backward 3: dY per tile, dX = dY W, dW += dY^T X, db += sum dY ---------------------------------------------------------
template <int CIN, int COUT, bool DX, bool DW>
__global__ __launch_bounds__(256) void pwt_backward_gemm_kernel(PwtBwdArgs a) {
    constexpr int LDO = COUT + TT_PAD, LDI = CIN + TT_PAD, C4N = COUT / 4, RL = 256 / C4N;
    constexpr int NTI = CIN / 64;                            // dX: 32-column blocks per wave
    constexpr int CIB = CIN / 32, TPW = (COUT / 32) * CIB / 4;   // dW: 32 x 32 blocks per wave
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float* dYs = lds;                                        // [64][LDO]
    float* Xs = dYs + TT_BM * LDO;                          // [64][LDI]    (DW)
    float* Ws = Xs + (DW ? TT_BM * LDI : 0);                // [COUT][LDI]  (DX)
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, l31 = lane & 31, h = lane >> 5;
    const int c4 = (t % C4N) * 4, rl = t / C4N;
    const int tiles = ceil_div_dev(a.M, TT_BM);

    float mu[4], is[4], ga[4], be[4], dbs[4];
    double mud[4], isd[4], k1[4], mb[4], mg[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        mud[e] = a.mean[c4 + e]; isd[e] = a.invstd[c4 + e]; ga[e] = a.gamma[c4 + e]; be[e] = a.beta[c4 + e];
        mu[e] = (float)mud[e]; is[e] = (float)isd[e];
        k1[e] = (double)ga[e] * isd[e];
        mb[e] = a.means[c4 + e];
        mg[e] = a.means[COUT + c4 + e];
        dbs[e] = 0.f;
    }
    if (DX) tt_stage_rows16<CIN>(a.W, 0, Ws, COUT, COUT);
    f32x16 accw[TPW];
    tt_zero(accw);

    for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int m0 = tile * TT_BM;
        const int nrows = min(TT_BM, a.M - m0);
        __syncthreads();                                     // the previous tile's readers are done
#pragma unroll
        for (int i = 0; i < TT_BM / RL; ++i) {
            const int r = rl + RL * i;
            f32x4 dy = {0.f, 0.f, 0.f, 0.f};
            if (r < nrows) {
                const f32x4 y = *reinterpret_cast<const f32x4*>(a.Y + (size_t)(m0 + r) * COUT + c4);
                const f32x4 dz = *reinterpret_cast<const f32x4*>(a.dZ + (size_t)(m0 + r) * COUT + c4);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float g = pwt_preact(pwt_xhat(y[e], mu[e], is[e]), ga[e], be[e]) > 0.f ? dz[e] : 0.f;
                    const float v = (float)(k1[e] * (((double)g - mb[e]) - pwt_xhat_f64(y[e], mud[e], isd[e]) * mg[e]));
                    dy[e] = v;
                    dbs[e] += v;
                }
            }
            *reinterpret_cast<f32x4*>(dYs + r * LDO + c4) = dy;
        }
        if (DW) tt_stage_rows16<CIN>(a.X, m0, Xs, TT_BM, nrows);
        __syncthreads();

        if (DX) {
            // dX[m][ci] = sum_co dY[m][co] W[co][ci]
            const int wm = wave & 1, wn = wave >> 1;
            f32x16 acc[NTI];
            tt_zero(acc);
            tt_mma_rows_cols<COUT, NTI, 2>(dYs + wm * 32 * LDO, LDO, Ws + wn * NTI * 32, LDI, acc);
#pragma unroll
            for (int nt = 0; nt < NTI; ++nt) {
                const int n = (wn * NTI + nt) * 32 + l31;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int i = wm * 32 + tt_acc_row(r, h);
                    if (i < nrows) a.dX[(size_t)(m0 + i) * CIN + n] = acc[nt][r];
                }
            }
        }
        // dW[co][ci] += sum_rows dY[row][co] X[row][ci]: block (co, ci) = (j / CIB, j % CIB)
        if (DW) tt_mma_cols_cols<TT_BM, TPW, CIB, 4>(dYs, LDO, Xs, LDI, wave * TPW, accw);
    }

    if (DW) {
        float* P = a.dwpart + (size_t)blockIdx.x * (COUT * CIN + COUT);
        tt_write_dw_blocks<TPW, CIB>(P, CIN, CIN, wave * TPW, accw);
        const float s = tt_column_sums<RL, COUT>(dYs, dbs, rl, c4, 1);      // db; the dY tile has no readers left
        if (t < COUT) P[COUT * CIN + t] = s;
    }
}

template <int CIN, int COUT>
static int pwt_launch_forward_gemm(const PwtFwdArgs& a, hipStream_t st) {
    return launch_with_dynamic_lds(pwt_forward_gemm_kernel<CIN, COUT>, dim3(tt_tiles(a.M)), (size_t)(TT_BM + COUT) * (CIN + TT_PAD) * sizeof(float),
                                   st, "pdsc_pointwise_train_forward", a);
}

template <int CIN, int COUT, bool DX, bool DW>
static int pwt_launch_backward_gemm(const PwtBwdArgs& a, hipStream_t st) {
    const size_t lds_floats = (size_t)TT_BM * (COUT + TT_PAD) + (DW ? TT_BM * (CIN + TT_PAD) : 0) + (DX ? COUT * (CIN + TT_PAD) : 0);
    return launch_with_dynamic_lds(pwt_backward_gemm_kernel<CIN, COUT, DX, DW>, dim3(tt_groups(a.M)), lds_floats * sizeof(float), st,
                                   "pdsc_pointwise_train_backward", a);
}

template <int CIN, int COUT>
static int pwt_launch_backward_gemm_select(const PwtBwdArgs& a, bool dx, bool dw, hipStream_t st) {
    if (dx && dw) return pwt_launch_backward_gemm<CIN, COUT, true, true>(a, st);
    if (dx) return pwt_launch_backward_gemm<CIN, COUT, true, false>(a, st);
    return pwt_launch_backward_gemm<CIN, COUT, false, true>(a, st);
}

}  // namespace pdsc

extern "C" size_t pdsc_pointwise_train_workspace_bytes(int M, int Cin, int Cout) {
    if (M < 2 || !pdsc::pwt_shape_ok(Cin, Cout)) return 0;
    return pdsc::pwt_part_bytes(M, Cout) + pdsc::pwt_sums_bytes(Cout) + pdsc::pwt_dw_bytes(M, Cin, Cout);
}

using pdsc::aligned16;

extern "C" int pdsc_pointwise_train_forward(const float* X, const float* W, const float* b, const float* gamma, const float* beta,
                                            float* running_mean, float* running_var, float momentum, float eps, float* Y, float* Z,
                                            double* mean, double* invstd, void* ws, size_t ws_bytes, int M, int Cin, int Cout,
                                            void* stream) {
    PDSC_REQUIRE(X && W && b && gamma && beta && running_mean && running_var && Y && Z && mean && invstd,
                 "pdsc_pointwise_train_forward: null pointer");
    PDSC_REQUIRE(pdsc::pwt_shape_ok(Cin, Cout), "pdsc_pointwise_train_forward: (Cin, Cout) = (%d, %d); supported: (128,128) (128,64) (64,64)",
                 Cin, Cout);
    PDSC_REQUIRE(M >= 2, "pdsc_pointwise_train_forward: M=%d (batch statistics need at least 2 rows)", M);
    PDSC_REQUIRE(momentum >= 0.f && momentum <= 1.f && eps >= 0.f, "pdsc_pointwise_train_forward: momentum=%g eps=%g", (double)momentum,
                 (double)eps);
    PDSC_REQUIRE(aligned16(X) && aligned16(W) && aligned16(Y) && aligned16(Z),
                 "pdsc_pointwise_train_forward: X, W, Y, Z must be 16-byte aligned");
    PDSC_REQUIRE(ws && (((uintptr_t)ws | (uintptr_t)mean | (uintptr_t)invstd) & 7) == 0,
                 "pdsc_pointwise_train_forward: workspace, mean and invstd must be 8-byte aligned");
    int rc = pdsc::check_workspace("pdsc_pointwise_train_forward", ws_bytes, pdsc_pointwise_train_workspace_bytes(M, Cin, Cout));
    if (rc != PDSC_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    pdsc::PwtFwdArgs a{};
    a.X = X; a.W = W; a.b = b; a.Y = Y; a.part = (double*)ws; a.M = M;
    if (Cin == 128 && Cout == 128) rc = pdsc::pwt_launch_forward_gemm<128, 128>(a, st);
    else if (Cin == 128) rc = pdsc::pwt_launch_forward_gemm<128, 64>(a, st);
    else rc = pdsc::pwt_launch_forward_gemm<64, 64>(a, st);
    if (rc != PDSC_OK) return rc;
    hipLaunchKernelGGL(pdsc::pwt_stats_merge_kernel, dim3(Cout / pdsc::PWT_MERGE_COLS), dim3(pdsc::PWT_MERGE_THREADS), 0, st, a.part, pdsc::tt_tiles(M), M, Cout,
                       momentum, eps, running_mean, running_var, mean, invstd);
    const int rows_per_block = 256 / (Cout / 4);
    int blocks = pdsc::ceil_div(M, rows_per_block * 4);
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(pdsc::pwt_norm_relu_kernel, dim3(blocks), dim3(256), 0, st, Y, mean, invstd, gamma, beta, Z, M, Cout);
    return pdsc::check_launch("pdsc_pointwise_train_forward(statistics, normalise)");
}

extern "C" int pdsc_pointwise_train_backward(const float* X, const float* W, const float* gamma, const float* beta, const float* Y,
                                             const double* mean, const double* invstd, const float* dZ, float* dX, float* dW, float* db,
                                             float* dgamma, float* dbeta, void* ws, size_t ws_bytes, int M, int Cin, int Cout,
                                             void* stream) {
    PDSC_REQUIRE(X && W && gamma && beta && Y && mean && invstd && dZ, "pdsc_pointwise_train_backward: null pointer");
    PDSC_REQUIRE(dX || dW || db || dgamma || dbeta, "pdsc_pointwise_train_backward: no gradient asked for");
    PDSC_REQUIRE(pdsc::pwt_shape_ok(Cin, Cout), "pdsc_pointwise_train_backward: (Cin, Cout) = (%d, %d); supported: (128,128) (128,64) (64,64)",
                 Cin, Cout);
    PDSC_REQUIRE(M >= 2, "pdsc_pointwise_train_backward: M=%d (batch statistics need at least 2 rows)", M);
    PDSC_REQUIRE(aligned16(X) && aligned16(W) && aligned16(Y) && aligned16(dZ) && aligned16(dX),
                 "pdsc_pointwise_train_backward: X, W, Y, dZ, dX must be 16-byte aligned");
    PDSC_REQUIRE(ws && (((uintptr_t)ws | (uintptr_t)mean | (uintptr_t)invstd) & 7) == 0,
                 "pdsc_pointwise_train_backward: workspace, mean and invstd must be 8-byte aligned");
    int rc = pdsc::check_workspace("pdsc_pointwise_train_backward", ws_bytes, pdsc_pointwise_train_workspace_bytes(M, Cin, Cout));
    if (rc != PDSC_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    double* part = (double*)ws;
    double* sums = (double*)((char*)ws + pdsc::pwt_part_bytes(M, Cout));
    float* dwpart = (float*)((char*)sums + pdsc::pwt_sums_bytes(Cout));
    const int tiles = pdsc::tt_tiles(M);
    if (Cout == 128)
        hipLaunchKernelGGL(pdsc::pwt_backward_reduce_kernel<128>, dim3(tiles), dim3(256), 0, st, Y, dZ, mean, invstd, gamma, beta, part, M);
    else
        hipLaunchKernelGGL(pdsc::pwt_backward_reduce_kernel<64>, dim3(tiles), dim3(256), 0, st, Y, dZ, mean, invstd, gamma, beta, part, M);
    hipLaunchKernelGGL(pdsc::pwt_sum_partials_kernel, dim3(2 * Cout / pdsc::PWT_MERGE_COLS), dim3(pdsc::PWT_MERGE_THREADS), 0, st, part, tiles, 2 * Cout, M, sums, dbeta,
                       dgamma);
    rc = pdsc::check_launch("pdsc_pointwise_train_backward(dbeta, dgamma)");
    if (rc != PDSC_OK) return rc;
    const bool want_dw = dW || db;
    if (!dX && !want_dw) return PDSC_OK;
    pdsc::PwtBwdArgs a{};
    a.X = X; a.W = W; a.Y = Y; a.dZ = dZ; a.mean = mean; a.invstd = invstd; a.gamma = gamma; a.beta = beta;
    a.means = sums; a.dX = dX; a.dwpart = dwpart; a.M = M;
    if (Cin == 128 && Cout == 128) rc = pdsc::pwt_launch_backward_gemm_select<128, 128>(a, dX != nullptr, want_dw, st);
    else if (Cin == 128) rc = pdsc::pwt_launch_backward_gemm_select<128, 64>(a, dX != nullptr, want_dw, st);
    else rc = pdsc::pwt_launch_backward_gemm_select<64, 64>(a, dX != nullptr, want_dw, st);
    if (rc != PDSC_OK || !want_dw) return rc;
    pdsc::TtMergeSegs sg{};
    sg.add(0, 0, Cout * Cin, dW);
    sg.add(0, Cout * Cin, Cout * Cin + Cout, db);
    return pdsc::tt_launch_merge(dwpart, pdsc::tt_groups(M), Cout * Cin + Cout, 1, sg, st, "pdsc_pointwise_train_backward(dW merge)");
}
