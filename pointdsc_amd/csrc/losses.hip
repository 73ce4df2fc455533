// f-11: the losses of libs/loss.py on the device, with their gradients -- what the reference's validation and training loops
// (libs/trainer.py:95-107,186-194) apply to the outputs of the validation forward.
//   pdsc_classification_loss   libs/loss.py:85-102   (BCE with logits in three weightings + the precision / recall / F1 row)
//   pdsc_sm_loss_matrix        libs/loss.py:129-138  on a stored M
//   pdsc_sm_loss_features      the same loss of M = clamp(1 - (1 - F F^T) / sigma^2, 0, 1) straight from F: M is never stored
//   pdsc_transformation_loss   libs/loss.py:34-63    (+ pdsc_transformation_loss_grad: its gradient with respect to trans, f-14)
// Determinism: no floating-point atomics anywhere.  Every workgroup reduces in a fixed tree (wave shuffle, then the waves in order)
// and writes fp64 partials into the workspace; a one-workgroup finishing launch adds them in index order.
//
// The two spectral-matching kernels share ONE element order, so that the features form equals the matrix form bit for bit on the
// matrix pdsc_feature_compat writes: a wavefront owns 32 indices a (lane & 31) and walks 32-index tiles of the other index o; per
// tile a lane holds the 16 elements o = tile * 32 + (r & 3) + 8 (r >> 2) + 4 (lane >> 5), r = 0..15 -- the accumulator layout of
// v_mfma_f32_32x32x2_f32 -- and adds them to its fp64 sums in r order.  In the features kernel the element is s(a, o) = <F_a, F_o>,
// computed with the tile's rows F_o as the A operand and the wave's own rows F_a as the B operand, by the tile function and the
// clamp expression gram_rows_kernel (linear.hip) uses (gram_tile.h: one text for both); in the matrix kernel it is M[o][a],
// which a half wave reads as 128 contiguous bytes -- and which pdsc_feature_compat computed with exactly these operand roles (A = row o, B = column a), so no symmetry of the matrix
// instruction is assumed.  The classes (gt_a gt_o, a != o) are symmetric in a and o, so for that M the two kernels add the same
// numbers in the same order.
//
// Why the roles are swapped: with accumulator lane = own row a and register = column o, the gradient tile g(a, o) is ALREADY an A
// operand of the second product dF_a += sum_o g(a, o) F_o (k slot (step r, half h) <-> o = (r & 3) + 8 (r >> 2) + 4 h): it goes
// from the accumulator registers into the MFMA without passing through LDS; the B operand F_o[channel] comes from the staged tile.
#include "pdsc_common.h"
#include "gram_tile.h"

namespace pdsc {

// block-wide fp64 sum of NV values per thread in a fixed order (wave shuffle tree, then waves 0..3); valid in every thread
template <int NV>
__device__ __forceinline__ void block_sum_f64(double (&v)[NV], double* red) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < NV; ++i) v[i] = wave_sum(v[i]);
    __syncthreads();
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < NV; ++i) red[wave * NV + i] = v[i];
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NV; ++i) v[i] = ((red[0 * NV + i] + red[1 * NV + i]) + red[2 * NV + i]) + red[3 * NV + i];
}

// ---------------------------------------------------------------------------------------------------------------------------
// classification loss
// ---------------------------------------------------------------------------------------------------------------------------
constexpr int CLS_NQ = 10, CLS_MAX_BLOCKS = 256;
// partial sums: 0 sum (1-y) softplus(x), 1 sum y softplus(-x), 2 sum w bce, 3 sum y, 4 sum (1-y), 5 sum x y, 6 sum x (1-y),
//               7 true positives, 8 predicted positives, 9 gt positives (7-9: pair 0 only)
__global__ __launch_bounds__(256) void cls_partial_kernel(const float* __restrict__ pred, const float* __restrict__ gt,
                                                          const float* __restrict__ weight, double* __restrict__ part, long long total,
                                                          int N) {
    __shared__ double red[4 * CLS_NQ];
    double v[CLS_NQ];
#pragma unroll
    for (int q = 0; q < CLS_NQ; ++q) v[q] = 0.0;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
        const float xf = pred[e], yf = gt[e];
        const double x = (double)xf, y = (double)yf;
        const double l = log1p(exp(-fabs(x)));
        const double neg = (1.0 - y) * (l + fmax(x, 0.0));       // (1 - y) softplus(x)  == (1 - y) (x + softplus(-x))
        const double pos = y * (l + fmax(-x, 0.0));              // y softplus(-x)
        v[0] += neg;
        v[1] += pos;
        if (weight) v[2] += (neg + pos) * (double)weight[e];
        v[3] += y;
        v[4] += 1.0 - y;
        v[5] += x * y;
        v[6] += x * (1.0 - y);
        if (e < N) {
            const bool p = xf > 0.f, g = yf == 1.0f;
            v[7] += (p && g) ? 1.0 : 0.0;
            v[8] += p ? 1.0 : 0.0;
            v[9] += g ? 1.0 : 0.0;
        }
    }
    block_sum_f64<CLS_NQ>(v, red);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int q = 0; q < CLS_NQ; ++q) part[(size_t)blockIdx.x * CLS_NQ + q] = v[q];
    }
}

__global__ __launch_bounds__(64) void cls_finish_kernel(const double* __restrict__ part, int blocks, long long total, int weighted,
                                                        int balanced, double* __restrict__ stats) {
    __shared__ double s[CLS_NQ];
    if (threadIdx.x < CLS_NQ) {
        double acc = 0.0;
        for (int b = 0; b < blocks; ++b) acc += part[(size_t)b * CLS_NQ + threadIdx.x];
        s[threadIdx.x] = acc;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    const double num_pos = fmax(s[3] - 1.0, 0.0) + 1.0, num_neg = fmax(s[4] - 1.0, 0.0) + 1.0;
    double loss;
    if (weighted) loss = s[2] / (double)total;
    else if (!balanced) loss = (s[0] + s[1]) / (double)total;
    else loss = (s[0] + (num_neg * 1.0 / num_pos) * s[1]) / (double)total;
    const double tp = s[7], pp = s[8], gp = s[9];
    stats[0] = loss;
    stats[1] = pp > 0.0 ? tp / pp : 0.0;                         // sklearn: 0 where nothing is predicted / labelled positive
    stats[2] = gp > 0.0 ? tp / gp : 0.0;
    stats[3] = (pp + gp) > 0.0 ? 2.0 * tp / (pp + gp) : 0.0;
    stats[4] = s[5] / fmax(1.0, s[3]);
    stats[5] = s[6] / fmax(1.0, s[4]);
    stats[6] = num_pos;
    stats[7] = num_neg;
}

// d loss / d pred; reads num_pos / num_neg from the stats row the finishing launch wrote
__global__ __launch_bounds__(256) void cls_grad_kernel(const float* __restrict__ pred, const float* __restrict__ gt,
                                                       const float* __restrict__ weight, const double* __restrict__ stats, int balanced,
                                                       double* __restrict__ dpred, long long total) {
    const double pw = (!weight && balanced) ? stats[7] * 1.0 / stats[6] : 1.0;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
        const double x = (double)pred[e], y = (double)gt[e];
        const double sig_pos = 1.0 / (1.0 + exp(-x)), sig_neg = 1.0 / (1.0 + exp(x));       // sigmoid(x), sigmoid(-x)
        double g = (1.0 - y) * sig_pos - pw * (y * sig_neg);
        if (weight) g *= (double)weight[e];
        dpred[e] = g / (double)total;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// spectral-matching loss
// ---------------------------------------------------------------------------------------------------------------------------
constexpr int SM_ROWS = 128, SM_TILE = 32, SM_LD = PDSC_CHANNELS + 4, SM_NP = 4;      // partial: sum_pos, sum_neg, dsigma sum, k

__device__ __forceinline__ bool sm_label(float g) { return g == 1.0f; }

// number of inliers of the pair (every thread gets it)
__device__ __forceinline__ int sm_count_inliers(const float* __restrict__ gt, int N, int* red) {
    int c = 0;
    for (int i = threadIdx.x; i < N; i += 256) c += sm_label(gt[i]) ? 1 : 0;
    c = wave_sum(c);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = c;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}

// class sizes of a pair with k inliers (the diagonal is negative): P = relu(k (k - 1) - 1) + 1, Q = relu(N^2 - k (k - 1) - 1) + 1
__device__ __forceinline__ void sm_class_sizes(int k, int N, double& P, double& Q) {
    const long long kk = (long long)k * (k - 1), nn = (long long)N * N;
    P = (double)((kk - 1 > 0 ? kk - 1 : 0) + 1);
    Q = (double)((nn - kk - 1 > 0 ? nn - kk - 1 : 0) + 1);
}

// one element into the lane's fp64 sums: the ONE definition both kernels use
__device__ __forceinline__ void sm_accumulate(float m, bool valid, bool pos, double& sp, double& sn) {
    const double d = (double)m, e = d - 1.0;
    sp += (valid && pos) ? e * e : 0.0;
    sn += (valid && !pos) ? d * d : 0.0;
}

__device__ __forceinline__ void sm_write_partial(double sp, double sn, double dsg, int k, double* red, double* part) {
    double v[3] = {sp, sn, dsg};
    block_sum_f64<3>(v, red);
    if (threadIdx.x == 0) { part[0] = v[0]; part[1] = v[1]; part[2] = v[2]; part[3] = (double)k; }
}

template <bool GRAD>
__global__ __launch_bounds__(256) void sm_loss_matrix_kernel(const float* __restrict__ M, long long ld, const float* __restrict__ gt_all,
                                                        int balanced, double* __restrict__ part, double* __restrict__ dM, int bs, int N) {
    __shared__ double red[4 * 3];
    __shared__ int redi[4];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, l31 = lane & 31, h = lane >> 5;
    const int b = blockIdx.y, rb = blockIdx.x;
    const float* gt = gt_all + (size_t)b * N;
    const float* Mb = M + (size_t)b * N * ld;
    const int k = sm_count_inliers(gt, N, redi);
    double cp = 0.0, cn = 0.0;
    if (GRAD) {
        double P, Q;
        sm_class_sizes(k, N, P, Q);
        cp = balanced ? 0.5 / (P * (double)bs) : 1.0 / ((double)bs * (double)N * (double)N);
        cn = balanced ? 0.5 / (Q * (double)bs) : cp;
    }
    const int a = rb * SM_ROWS + wave * 32 + l31;
    const bool va = a < N;
    const bool ga = sm_label(gt[min(a, N - 1)]);
    double sp = 0.0, sn = 0.0;
    const int tiles = ceil_div_dev(N, SM_TILE);
    for (int tile = 0; tile < tiles; ++tile) {
        float m[16];
        bool go[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int o = tile * SM_TILE + (r & 3) + 8 * (r >> 2) + 4 * h;
            const bool valid = va && o < N;
            m[r] = valid ? Mb[(size_t)o * ld + a] : 0.f;
            go[r] = sm_label(gt[min(o, N - 1)]);
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int o = tile * SM_TILE + (r & 3) + 8 * (r >> 2) + 4 * h;
            const bool valid = va && o < N;
            const bool pos = ga && go[r] && a != o;
            sm_accumulate(m[r], valid, pos, sp, sn);
            if (GRAD && valid) dM[((size_t)b * N + o) * ld + a] = (pos ? cp : cn) * (2.0 * ((double)m[r] - (pos ? 1.0 : 0.0)));
        }
    }
    sm_write_partial(sp, sn, 0.0, k, red, part + ((size_t)b * gridDim.x + rb) * SM_NP);
}

struct SmFeatArgs {
    const float* X;          // [bs][N][128]
    const float* sigma;
    const float* gt;         // [bs][N]
    double* part;            // [bs][row blocks][SM_NP]
    float* dnormed;          // [bs][N][128] or NULL
    int bs, N, balanced;
};

template <bool GRAD>
__global__ __launch_bounds__(256) void sm_loss_features_kernel(SmFeatArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];       // 2 x [SM_TILE][SM_LD]
    __shared__ double red[4 * 3];
    __shared__ int redi[4];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, l31 = lane & 31, h = lane >> 5;
    const int b = blockIdx.y, rb = blockIdx.x, N = a.N;
    const float* X = a.X + (size_t)b * N * PDSC_CHANNELS;
    const float* gt = a.gt + (size_t)b * N;
    const int k = sm_count_inliers(gt, N, redi);
    float cp = 0.f, cn = 0.f;
    if (GRAD) {
        double P, Q;
        sm_class_sizes(k, N, P, Q);
        const double cu = 1.0 / ((double)a.bs * (double)N * (double)N);
        cp = (float)(a.balanced ? 0.5 / (P * (double)a.bs) : cu);
        cn = (float)(a.balanced ? 0.5 / (Q * (double)a.bs) : cu);
    }
    const float sg = a.sigma[0], sig2 = sg * sg;

    // this lane's own row: B fragments, k-slot (4q+e, half h) <-> channel 8q+4h+e (the convention of linear.hip)
    const int i = rb * SM_ROWS + wave * 32 + l31;
    const bool vi = i < N;
    const bool gi = sm_label(gt[min(i, N - 1)]);
    f32x4 bf[16];
    {
        const float* p = X + (size_t)min(i, N - 1) * PDSC_CHANNELS + 4 * h;
#pragma unroll
        for (int q = 0; q < 16; ++q) bf[q] = *reinterpret_cast<const f32x4*>(p + 8 * q);
    }
    // stage loader: thread -> 4 float4 of a 32 x 128 tile (rows past N repeat row N - 1: finite values under a zero gradient)
    f32x4 stage[4];
    auto load_tile = [&](int tile) {
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int f = t + 256 * s, r = f >> 5, c4 = (f & 31) * 4;
            const int col = min(tile * SM_TILE + r, N - 1);
            stage[s] = *reinterpret_cast<const f32x4*>(X + (size_t)col * PDSC_CHANNELS + c4);
        }
    };
    auto store_tile = [&](float* buf) {
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int f = t + 256 * s, r = f >> 5, c4 = (f & 31) * 4;
            *reinterpret_cast<f32x4*>(buf + r * SM_LD + c4) = stage[s];
        }
    };
    f32x16 dF[4];                                   // GRAD: 32 rows x 128 channels of sum_o g(i, o) F_o, 4 accumulator tiles
    if (GRAD) {
#pragma unroll
        for (int cb = 0; cb < 4; ++cb)
#pragma unroll
            for (int r = 0; r < 16; ++r) dF[cb][r] = 0.f;
    }
    double sp = 0.0, sn = 0.0, dsg = 0.0;
    const int tiles = ceil_div_dev(N, SM_TILE);
    load_tile(0);
    store_tile(lds);
    __syncthreads();
    for (int tile = 0; tile < tiles; ++tile) {
        const float* cur = lds + (tile & 1) * SM_TILE * SM_LD;
        if (tile + 1 < tiles) load_tile(tile + 1);                       // in flight under the MFMAs
        bool go[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) go[r] = sm_label(gt[min(tile * SM_TILE + (r & 3) + 8 * (r >> 2) + 4 * h, N - 1)]);
        const f32x16 acc = gram_tile_k128<false>(bf, cur + l31 * SM_LD + 4 * h);      // gram_tile.h: A = the tile's rows, B = own rows
        float g[16];
        float dsg_tile = 0.f;                       // fp32 over the 16 elements of one tile column, fp64 above
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int o = tile * SM_TILE + (r & 3) + 8 * (r >> 2) + 4 * h;
            const bool valid = vi && o < N;
            const float s = acc[r];
            const float raw = feature_compat_raw(s, sig2);
            float m = feature_compat_clamp(raw);                        // gram_tile.h: the expression gram_rows_kernel MODE 2 stores
            if (i == o) m = 0.0f;
            const bool pos = gi && go[r] && i != o;
            sm_accumulate(m, valid, pos, sp, sn);
            if (GRAD) {
                const bool live = valid && i != o && raw >= 0.0f && raw <= 1.0f;     // inclusive: torch.clamp's backward
                const float gv = live ? (pos ? cp : cn) * (2.0f * (m - (pos ? 1.0f : 0.0f))) : 0.0f;
                g[r] = gv;
                dsg_tile += gv * (1.0f - s);
            }
        }
        if (GRAD) {
            dsg += (double)dsg_tile;
            // dF[i][c] += sum_o g(i, o) F_o[c]: A = g straight from the registers (lane = i, k slot (r, h) <-> o), B = the staged tile
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float* frow = cur + ((r & 3) + 8 * (r >> 2) + 4 * h) * SM_LD + l31;
#pragma unroll
                for (int cb = 0; cb < 4; ++cb) dF[cb] = __builtin_amdgcn_mfma_f32_32x32x2f32(g[r], frow[32 * cb], dF[cb], 0, 0, 0);
            }
        }
        if (tile + 1 < tiles) {
            store_tile(lds + ((tile + 1) & 1) * SM_TILE * SM_LD);       // the other buffer: its readers finished a barrier ago
            __syncthreads();
        }
    }
    if (GRAD && a.dnormed) {
        const float scale = 2.0f / sig2;
        float* D = a.dnormed + (size_t)b * N * PDSC_CHANNELS;
#pragma unroll
        for (int cb = 0; cb < 4; ++cb)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = rb * SM_ROWS + wave * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;       // accumulator lane = channel
                if (row < N) D[(size_t)row * PDSC_CHANNELS + 32 * cb + l31] = scale * dF[cb][r];
            }
    }
    sm_write_partial(sp, sn, dsg, k, red, a.part + ((size_t)b * gridDim.x + rb) * SM_NP);
}

// pairs: ws[0 .. bs) = l_b (and, behind them, the pairs' dsigma sums); loss = mean_b l_b; dsigma = (2 / sigma^3) sum_b sum_rb
__global__ __launch_bounds__(256) void sm_loss_finish_kernel(const double* __restrict__ part, int row_blocks, int bs, int N, int balanced,
                                                        const float* __restrict__ sigma, double* __restrict__ pair_vals,
                                                        double* __restrict__ pair_dsg, double* __restrict__ loss,
                                                        double* __restrict__ dsigma) {
    for (int b = threadIdx.x; b < bs; b += 256) {
        double sp = 0.0, sn = 0.0, dsg = 0.0;
        for (int rb = 0; rb < row_blocks; ++rb) {
            const double* p = part + ((size_t)b * row_blocks + rb) * SM_NP;
            sp += p[0]; sn += p[1]; dsg += p[2];
        }
        double P, Q;
        sm_class_sizes((int)part[(size_t)b * row_blocks * SM_NP + 3], N, P, Q);
        pair_vals[b] = balanced ? 0.5 * sp / P + 0.5 * sn / Q : (sp + sn) / ((double)N * (double)N);
        pair_dsg[b] = dsg;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    double l = 0.0, d = 0.0;
    for (int b = 0; b < bs; ++b) { l += pair_vals[b]; d += pair_dsg[b]; }
    loss[0] = l / (double)bs;
    if (dsigma) {
        const double sg = (double)sigma[0];
        dsigma[0] = d * 2.0 / (sg * sg * sg);
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// transformation loss
// ---------------------------------------------------------------------------------------------------------------------------
constexpr int TR_MAX_CHUNKS = 64, TR_NP = 3;        // partial: sum of norms, sum of squared norms, #probs > 0

// block (chunk, i): pair i's warped source rows against the target rows of EVERY pair (the reference's broadcast)
__global__ __launch_bounds__(256) void trans_partial_kernel(const float* __restrict__ trans, const float* __restrict__ src,
                                                            const float* __restrict__ tgt, const float* __restrict__ probs,
                                                            double* __restrict__ part, int bs, int N) {
    __shared__ double red[4 * TR_NP];
    const int i = blockIdx.y;
    const float* T = trans + (size_t)i * 16;
    double R[3][3], tv[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int c = 0; c < 3; ++c) R[r][c] = (double)T[r * 4 + c];
        tv[r] = (double)T[r * 4 + 3];
    }
    const long long total = (long long)bs * N;
    double v[TR_NP] = {0.0, 0.0, 0.0};
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
        const int n = (int)(e % N);
        const float* s = src + ((size_t)i * N + n) * 3;
        const float* g = tgt + (size_t)e * 3;
        const double sx = (double)s[0], sy = (double)s[1], sz = (double)s[2];
        double sq = 0.0;
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const double w = ((R[r][0] * sx + R[r][1] * sy) + R[r][2] * sz) + tv[r];
            const double d = w - (double)g[r];
            sq += d * d;
        }
        v[0] += sqrt(sq);
        v[1] += sq;
        if (e < N) v[2] += probs[(size_t)i * N + e] > 0.f ? 1.0 : 0.0;
    }
    block_sum_f64<TR_NP>(v, red);
    if (threadIdx.x == 0) {
        double* p = part + ((size_t)i * gridDim.x + blockIdx.x) * TR_NP;
        p[0] = v[0]; p[1] = v[1]; p[2] = v[2];
    }
}

__global__ __launch_bounds__(256) void trans_finish_kernel(const float* __restrict__ trans, const float* __restrict__ gt_trans,
                                                           const double* __restrict__ part, int chunks, double* __restrict__ pair_vals,
                                                           float re_thre, float te_thre, double* __restrict__ out, int bs, int N) {
    for (int i = threadIdx.x; i < bs; i += 256) {
        const float* T = trans + (size_t)i * 16;
        const float* G = gt_trans + (size_t)i * 16;
        double tr = 0.0;                            // trace(R^T gR): columns in order, rows within a column in order
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int r = 0; r < 3; ++r) tr += (double)T[r * 4 + c] * (double)G[r * 4 + c];
        const double re = acos(fmin(fmax((tr - 1.0) / 2.0, -1.0), 1.0)) * 180.0 / 3.141592653589793;
        double tt = 0.0;
#pragma unroll
        for (int r = 0; r < 3; ++r) { const double d = (double)T[r * 4 + 3] - (double)G[r * 4 + 3]; tt += d * d; }
        const double te = sqrt(tt) * 100.0;
        double sn = 0.0, sq = 0.0, np = 0.0;
        for (int c = 0; c < chunks; ++c) {
            const double* p = part + ((size_t)i * chunks + c) * TR_NP;
            sn += p[0]; sq += p[1]; np += p[2];
        }
        const double rows = (double)bs * (double)N;
        double* o = pair_vals + (size_t)i * 5;
        o[0] = np > 0.0 ? sq / rows : 0.0;
        o[1] = (te < (double)te_thre && re < (double)re_thre) ? 1.0 : 0.0;
        o[2] = re; o[3] = te; o[4] = sn / rows;
    }
    __syncthreads();
    if (threadIdx.x >= 5) return;
    double acc = 0.0;
    for (int i = 0; i < bs; ++i) acc += pair_vals[(size_t)i * 5 + threadIdx.x];
    out[threadIdx.x] = threadIdx.x == 1 ? acc * 100.0 / (double)bs : acc / (double)bs;
}

// d loss / d trans[:, :3, :] of the value above (f-14): loss = (1 / bs) sum_i [some probs_i > 0] (1 / (bs N)) sum_(j,n) |R_i s_in + t_i - g_jn|^2,
// so d / dT_i[r][c] = (2 / (bs bs N)) sum_(j,n) d_r (s_c | 1).  Partial: the 12 sums of d_r (s_c | 1) and #probs > 0.
constexpr int TRG_NP = 13;
__global__ __launch_bounds__(256) void trans_grad_partial_kernel(const float* __restrict__ trans, const float* __restrict__ src,
                                                                 const float* __restrict__ tgt, const float* __restrict__ probs,
                                                                 double* __restrict__ part, int bs, int N) {
    __shared__ double red[4 * TRG_NP];
    const int i = blockIdx.y;
    const float* T = trans + (size_t)i * 16;
    double R[3][3], tv[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int c = 0; c < 3; ++c) R[r][c] = (double)T[r * 4 + c];
        tv[r] = (double)T[r * 4 + 3];
    }
    const long long total = (long long)bs * N;
    double v[TRG_NP];
#pragma unroll
    for (int q = 0; q < TRG_NP; ++q) v[q] = 0.0;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
        const int n = (int)(e % N);
        const float* s = src + ((size_t)i * N + n) * 3;
        const float* g = tgt + (size_t)e * 3;
        const double sx = (double)s[0], sy = (double)s[1], sz = (double)s[2];
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const double w = ((R[r][0] * sx + R[r][1] * sy) + R[r][2] * sz) + tv[r];
            const double d = w - (double)g[r];
            v[r * 4 + 0] += d * sx; v[r * 4 + 1] += d * sy; v[r * 4 + 2] += d * sz; v[r * 4 + 3] += d;
        }
        if (e < N) v[12] += probs[(size_t)i * N + e] > 0.f ? 1.0 : 0.0;
    }
    block_sum_f64<TRG_NP>(v, red);
    if (threadIdx.x == 0) {
        double* p = part + ((size_t)i * gridDim.x + blockIdx.x) * TRG_NP;
#pragma unroll
        for (int q = 0; q < TRG_NP; ++q) p[q] = v[q];
    }
}

// dtrans [bs][16]: the chunks added in index order; row 3 and the pairs without a positive prob are exact zeros
__global__ __launch_bounds__(256) void trans_grad_finish_kernel(const double* __restrict__ part, int chunks, double* __restrict__ dtrans,
                                                                int bs, int N) {
    for (int f = threadIdx.x; f < bs * 16; f += 256) {
        const int i = f >> 4, e = f & 15;
        double acc = 0.0, np = 0.0;
        for (int c = 0; c < chunks; ++c) {
            const double* p = part + ((size_t)i * chunks + c) * TRG_NP;
            if (e < 12) acc += p[e];
            np += p[12];
        }
        dtrans[f] = (e < 12 && np > 0.0) ? 2.0 * acc / ((double)bs * (double)N * (double)bs) : 0.0;
    }
}

static int sm_row_blocks(int N) { return ceil_div(N, SM_ROWS); }
static int trans_chunks(int bs, int N) {
    const long long c = ((long long)bs * N + 1023) / 1024;
    return (int)(c < TR_MAX_CHUNKS ? c : TR_MAX_CHUNKS);
}
static size_t loss_ws_doubles(int bs, int N) {
    const size_t sm = (size_t)2 * bs + (size_t)bs * sm_row_blocks(N) * SM_NP;
    const size_t cls = (size_t)CLS_MAX_BLOCKS * CLS_NQ;
    const size_t tr = (size_t)bs * 5 + (size_t)bs * trans_chunks(bs, N) * TR_NP;
    const size_t trg = (size_t)bs * trans_chunks(bs, N) * TRG_NP;
    size_t m = sm > cls ? sm : cls;
    m = m > tr ? m : tr;
    return m > trg ? m : trg;
}

}  // namespace pdsc

extern "C" size_t pdsc_loss_workspace_bytes(int bs, int N) {
    if (bs <= 0 || N <= 0) return 0;
    return pdsc::loss_ws_doubles(bs, N) * sizeof(double);
}

#define PDSC_LOSS_WS(name)                                                                                                      \
    PDSC_REQUIRE(bs > 0 && N > 0 && bs <= 65535, name ": bs=%d N=%d", bs, N);                                                   \
    PDSC_REQUIRE(ws && ((uintptr_t)ws & 7) == 0, name ": workspace must be 8-byte aligned");                                    \
    if (ws_bytes < pdsc_loss_workspace_bytes(bs, N)) {                                                                          \
        pdsc::set_error(name ": workspace of %zu bytes, needs %zu", ws_bytes, pdsc_loss_workspace_bytes(bs, N));                \
        return PDSC_ERR_WORKSPACE;                                                                                              \
    }

extern "C" int pdsc_classification_loss(const float* pred, const float* gt, const float* weight, int balanced, double* stats,
                                        double* dpred, void* ws, size_t ws_bytes, int bs, int N, void* stream) {
    PDSC_REQUIRE(pred && gt && stats, "pdsc_classification_loss: null pointer");
    PDSC_LOSS_WS("pdsc_classification_loss")
    hipStream_t st = (hipStream_t)stream;
    const long long total = (long long)bs * N;
    const long long want = (total + 1023) / 1024;
    const int blocks = (int)(want < pdsc::CLS_MAX_BLOCKS ? want : pdsc::CLS_MAX_BLOCKS);
    double* part = (double*)ws;
    hipLaunchKernelGGL(pdsc::cls_partial_kernel, dim3(blocks), dim3(256), 0, st, pred, gt, weight, part, total, N);
    hipLaunchKernelGGL(pdsc::cls_finish_kernel, dim3(1), dim3(64), 0, st, part, blocks, total, weight ? 1 : 0, balanced, stats);
    if (dpred)
        hipLaunchKernelGGL(pdsc::cls_grad_kernel, dim3(blocks), dim3(256), 0, st, pred, gt, weight, stats, balanced, dpred, total);
    return pdsc::check_launch("pdsc_classification_loss");
}

extern "C" int pdsc_sm_loss_matrix(const float* M, long long ld, const float* gt, int balanced, double* loss, double* dM, void* ws,
                                   size_t ws_bytes, int bs, int N, void* stream) {
    PDSC_REQUIRE(M && gt && loss, "pdsc_sm_loss_matrix: null pointer");
    PDSC_REQUIRE(ld >= N, "pdsc_sm_loss_matrix: ld=%lld < N=%d", ld, N);
    PDSC_LOSS_WS("pdsc_sm_loss_matrix")
    hipStream_t st = (hipStream_t)stream;
    const int rbs = pdsc::sm_row_blocks(N);
    double* pair_vals = (double*)ws;
    double* pair_dsg = pair_vals + bs;
    double* part = pair_dsg + bs;
    if (dM) hipLaunchKernelGGL(pdsc::sm_loss_matrix_kernel<true>, dim3(rbs, bs), dim3(256), 0, st, M, ld, gt, balanced, part, dM, bs, N);
    else hipLaunchKernelGGL(pdsc::sm_loss_matrix_kernel<false>, dim3(rbs, bs), dim3(256), 0, st, M, ld, gt, balanced, part, dM, bs, N);
    hipLaunchKernelGGL(pdsc::sm_loss_finish_kernel, dim3(1), dim3(256), 0, st, part, rbs, bs, N, balanced, (const float*)nullptr, pair_vals,
                       pair_dsg, loss, (double*)nullptr);
    return pdsc::check_launch("pdsc_sm_loss_matrix");
}

extern "C" int pdsc_sm_loss_features(const float* normed, const float* sigma, const float* gt, int balanced, double* loss,
                                     float* dnormed, double* dsigma, void* ws, size_t ws_bytes, int bs, int N, void* stream) {
    PDSC_REQUIRE(normed && sigma && gt && loss, "pdsc_sm_loss_features: null pointer");
    PDSC_REQUIRE(((uintptr_t)normed & 15) == 0, "pdsc_sm_loss_features: normed must be 16-byte aligned");
    PDSC_LOSS_WS("pdsc_sm_loss_features")
    hipStream_t st = (hipStream_t)stream;
    const int rbs = pdsc::sm_row_blocks(N);
    double* pair_vals = (double*)ws;
    double* pair_dsg = pair_vals + bs;
    pdsc::SmFeatArgs a{};
    a.X = normed; a.sigma = sigma; a.gt = gt; a.part = pair_dsg + bs; a.dnormed = dnormed; a.bs = bs; a.N = N; a.balanced = balanced;
    const size_t lds_bytes = 2 * (size_t)pdsc::SM_TILE * pdsc::SM_LD * sizeof(float);      // 33 792 B
    if (dnormed || dsigma) hipLaunchKernelGGL(pdsc::sm_loss_features_kernel<true>, dim3(rbs, bs), dim3(256), lds_bytes, st, a);
    else hipLaunchKernelGGL(pdsc::sm_loss_features_kernel<false>, dim3(rbs, bs), dim3(256), lds_bytes, st, a);
    hipLaunchKernelGGL(pdsc::sm_loss_finish_kernel, dim3(1), dim3(256), 0, st, a.part, rbs, bs, N, balanced, sigma, pair_vals, pair_dsg, loss,
                       dsigma);
    return pdsc::check_launch("pdsc_sm_loss_features");
}

extern "C" int pdsc_transformation_loss(const float* trans, const float* gt_trans, const float* src, const float* tgt,
                                        const float* probs, float re_thre, float te_thre, double* out, void* ws, size_t ws_bytes,
                                        int bs, int N, void* stream) {
    PDSC_REQUIRE(trans && gt_trans && src && tgt && probs && out, "pdsc_transformation_loss: null pointer");
    PDSC_LOSS_WS("pdsc_transformation_loss")
    hipStream_t st = (hipStream_t)stream;
    const int chunks = pdsc::trans_chunks(bs, N);
    double* pair_vals = (double*)ws;
    double* part = pair_vals + (size_t)bs * 5;
    hipLaunchKernelGGL(pdsc::trans_partial_kernel, dim3(chunks, bs), dim3(256), 0, st, trans, src, tgt, probs, part, bs, N);
    hipLaunchKernelGGL(pdsc::trans_finish_kernel, dim3(1), dim3(256), 0, st, trans, gt_trans, part, chunks, pair_vals, re_thre, te_thre,
                       out, bs, N);
    return pdsc::check_launch("pdsc_transformation_loss");
}

extern "C" int pdsc_transformation_loss_grad(const float* trans, const float* src, const float* tgt, const float* probs, double* dtrans,
                                             void* ws, size_t ws_bytes, int bs, int N, void* stream) {
    PDSC_REQUIRE(trans && src && tgt && probs && dtrans, "pdsc_transformation_loss_grad: null pointer");
    PDSC_LOSS_WS("pdsc_transformation_loss_grad")
    hipStream_t st = (hipStream_t)stream;
    const int chunks = pdsc::trans_chunks(bs, N);
    double* part = (double*)ws;
    hipLaunchKernelGGL(pdsc::trans_grad_partial_kernel, dim3(chunks, bs), dim3(256), 0, st, trans, src, tgt, probs, part, bs, N);
    hipLaunchKernelGGL(pdsc::trans_grad_finish_kernel, dim3(1), dim3(256), 0, st, part, chunks, dtrans, bs, N);
    return pdsc::check_launch("pdsc_transformation_loss_grad");
}
