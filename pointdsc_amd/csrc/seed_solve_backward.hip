// f-14: backward of the per-seed solver (solver.hip: k x k feature * spatial compatibility, power iteration, weighted Procrustes)
// for an upstream gradient of the seed hypotheses -- what lets a loss of final_trans reach the encoder and sigma.
//   reference: models/PointDSC.py:248-320 (cal_seed_trans, all of it under autograd), models/common.py:7-45 (rigid_transform_3d).
// ONE WAVEFRONT PER SEED, lane = neighbour, as seed_solve_kernel; a workgroup is one wavefront.  Nothing of the forward is read
// back but the early-exit mask: the wavefront rebuilds 1 - G (G = F F^T) and M, keeps them in wave-private LDS, replays the T
// iterates the forward chose (every v_t and ||u_t|| kept), redoes the weighted Procrustes, and walks the chain backwards.
// G is accumulated in fp64 and the spatial term takes the reference's roundings (ssb_spatial), unlike the forward's fp32 MFMA Gram
// and 1-ulp square roots: dsigma = sum dMf 2 (1 - G) / sigma^3 cancels heavily, and an fp32 Gram alone costs it 1e-5 of its value
// (profiles/f14_seed_solve_backward_errors.txt); M differs from the forward's in the last bits, the iterate count is the forward's.
//   t = cB - R cA                   -> dcB = dt, dcA = -R^T dt, dR -= dt cA^T
//   R = V diag(1,1,det) U^T         -> dH.  With A = H^T = R P, P = U diag(s') U^T symmetric, s' = (s1, s2, det s3):
//                                      R^T dA = Omega P + dP with Omega = R^T dR antisymmetric, so in the basis U
//                                      Omega~_ij = [U^T (R^T dA - dA^T R) U]_ij / (s'_i + s'_j); its adjoint for a gradient gR is
//                                      gA = R U Q U^T,  Q_ij = [U^T (Y - Y^T) U]_ij / (s'_i + s'_j) (i != j),  Y = R^T gR;  gH = gA^T
//   H, cA, cB (both + 1e-6 kept)    -> dw_i = am_i^T gH bm_i + (gcA . am_i + gcB . bm_i) / den, gcA -= gH sum w bm, gcB -= gH^T sum w am
//   w = v / (sum v + 1e-6)          -> dv_T
//   v_t = u_t / (||u_t|| + 1e-6)    -> du_t;   u_t = M v_{t-1} -> dM += du_t v_{t-1}^T, dv_{t-1} = M^T du_t      (t = T .. 1)
//   M = max(raw, 0) * M_spat, zero diagonal, raw = 1 - (1 - G) / sigma^2
//                                   -> dMf = [raw >= 0][i != j] dM * M_spat;  dsigma += sum dMf 2 (1 - G) / sigma^3;
//                                      dF_knn = (1 / sigma^2) (dMf + dMf^T) F_knn
// The Gram, the spatial term and the 3x3 part (the forward's Jacobi, extended by U and s') run in fp64 registers, the rest in fp32.
// Seeds whose twelve upstream values are all zero return at once (in training one seed per pair has a gradient).
// Determinism: no floating-point atomics.  A seed writes its k x 128 block and its fp64 dsigma term into the workspace; the owner
// pass gives every row of dnormed one wavefront that adds the blocks naming it in (seed, neighbour) order; one wavefront adds the
// dsigma terms in a fixed tree.  An entry of knn_idx outside [0, N) is never used as an address: it poisons that seed's block and
// dsigma term with NaN.  A seed whose u_t is the zero vector yields NaN (0 / 0), as torch's autograd does.
#include "pdsc_common.h"
#include "solver_common.h"

namespace pdsc {

// The spatial term max(1 - (|a_i - a_j| - |b_i - b_j|)^2 / sigma_d^2, 0) with the reference's roundings (models/PointDSC.py:268-272 on
// fp32 tensors): each distance is the correctly rounded fp32 square root (fp64 sum of squares, fp64 sqrt, one rounding), their
// difference and its square are fp32; the division and the clamp run in fp64.  Symmetric in (i, j) bit for bit.
__device__ __forceinline__ double ssb_spatial(float ax, float ay, float az, float bx, float by, float bz, const f32x4 pj, const f32x4 qj,
                                              double sd2) {
    const double dx = (double)ax - (double)pj[0], dy = (double)ay - (double)pj[1], dz = (double)az - (double)pj[2];
    const double ex = (double)bx - (double)qj[0], ey = (double)by - (double)qj[1], ez = (double)bz - (double)qj[2];
    const float ds = (float)sqrt((dx * dx + dy * dy) + dz * dz);
    const float dt = (float)sqrt((ex * ex + ey * ey) + ez * ez);
    const float df = ds - dt;
    return fmax(1.0 - (double)(df * df) / sd2, 0.0);
}

template <int NB>
struct SsbLds {
    static constexpr int KP = 16 * NB, MLD = KP + 1;
    float M[KP * MLD];                                   // M, then dMf
    float G[KP * MLD];                                   // 1 - F F^T, then dMf + dMf^T
    float pts[KP][8];
    float V[PDSC_MAX_POWER_ITERS + 1][KP];               // v_0 .. v_T
    float x[KP];                                         // du_t, broadcast
    float nrm[PDSC_MAX_POWER_ITERS + 1];                 // ||u_t||  (last: everything above stays 16-byte aligned)
};

struct SsbArgs {
    const float* normed; const float* src; const float* tgt; const int* knn_idx;
    const float* sigma; const float* sigma_spat; const unsigned int* conv_mask; const float* dtrans;
    float* blocks;           // [bs*S][k][128]
    double* part;            // [bs*S]
    int* active;             // [bs*S]
    int N, S, k, num_iter;
};

template <int NB>
__global__ __launch_bounds__(64) void seed_solve_backward_kernel(SsbArgs a) {
    using L = SsbLds<NB>;
    constexpr int KP = L::KP, MLD = L::MLD;
    __shared__ __attribute__((aligned(16))) L sh;
    const int lane = threadIdx.x, s = blockIdx.x, b = blockIdx.y;
    const int N = a.N, k = a.k;
    const size_t seed = (size_t)b * a.S + s;
    // the twelve upstream values (rows 0..2 of the row-major 4x4); all zero (or no iterate: v = 1, no path to the features): nothing to do
    float g = 0.f;
    if (lane < 12) g = a.dtrans[seed * 16 + lane];
    if (a.num_iter <= 0 || __builtin_amdgcn_ballot_w64(g != 0.0f) == 0ull) {
        if (lane == 0) a.active[seed] = 0;
        return;
    }
    const int T = chosen_iterate(a.conv_mask[b], a.num_iter) + 1;          // 1 .. num_iter
    const bool valid = lane < k;
    int idx = a.knn_idx[seed * k + (valid ? lane : 0)];
    const bool oob = (unsigned int)idx >= (unsigned int)N;
    const bool bad = __builtin_amdgcn_ballot_w64(oob) != 0ull;                   // never an address: the block becomes NaN below
    if (oob) idx = 0;
    const float* srcb = a.src + (size_t)b * N * 3;
    const float* tgtb = a.tgt + (size_t)b * N * 3;
    const float* nb = a.normed + (size_t)b * N * PDSC_CHANNELS;
    const float ax = srcb[idx * 3], ay = srcb[idx * 3 + 1], az = srcb[idx * 3 + 2];
    const float bx = tgtb[idx * 3], by = tgtb[idx * 3 + 1], bz = tgtb[idx * 3 + 2];
    if (lane < KP) {
        *reinterpret_cast<f32x4*>(&sh.pts[lane][0]) = f32x4{ax, ay, az, 0.f};
        *reinterpret_cast<f32x4*>(&sh.pts[lane][4]) = f32x4{bx, by, bz, 0.f};
    }
    const float sg = a.sigma[0], rsig2 = 1.0f / (sg * sg);
    const double sg2d = (double)sg * (double)sg, sd2d = (double)a.sigma_spat[0] * (double)a.sigma_spat[0];
    wave_lds_sync();
    {   // ---- 1 - G and M, row by row: lane = column j holds its own feature row as 128 doubles, row i's features arrive as wave-
        // uniform loads; G_ij is the fp64 chain over the channels in order, so G (and M) are symmetric bit for bit
        double fj[PDSC_CHANNELS];
        const float* own = nb + (size_t)idx * PDSC_CHANNELS;
#pragma unroll
        for (int c4 = 0; c4 < PDSC_CHANNELS / 4; ++c4) {
            const f32x4 t = *reinterpret_cast<const f32x4*>(own + 4 * c4);
#pragma unroll
            for (int e = 0; e < 4; ++e) fj[4 * c4 + e] = (double)t[e];
        }
        for (int i = 0; i < KP; ++i) {
            float m = 0.f, omg = 0.f;
            if (i < k) {                                              // (uniform)
                const int nbr = __builtin_amdgcn_readlane(idx, i);
                const float* row = nb + (size_t)nbr * PDSC_CHANNELS;
                double acc = 0.0;
#pragma unroll
                for (int c = 0; c < PDSC_CHANNELS; ++c) acc = fma((double)row[c], fj[c], acc);
                const double one_minus_g = 1.0 - acc;
                const f32x4 pi = *reinterpret_cast<const f32x4*>(&sh.pts[i][0]);
                const f32x4 qi = *reinterpret_cast<const f32x4*>(&sh.pts[i][4]);
                const double fm = fmax(1.0 - one_minus_g / sg2d, 0.0);
                omg = (float)one_minus_g;
                m = (i == lane || !valid) ? 0.0f : (float)(fm * ssb_spatial(ax, ay, az, bx, by, bz, pi, qi, sd2d));
            }
            if (lane < KP) { sh.M[i * MLD + lane] = m; sh.G[i * MLD + lane] = omg; }
        }
    }
    wave_lds_sync();
    const int rowl = min(lane, KP - 1);
    float mrow[KP];
#pragma unroll
    for (int j = 0; j < KP; ++j) mrow[j] = sh.M[rowl * MLD + j];
    // ---- replay: v_t = M v_{t-1} / (||M v_{t-1}|| + 1e-6), t = 1 .. T, all kept
    float v = valid ? 1.0f : 0.0f;
    if (lane < KP) sh.V[0][lane] = v;
    for (int t = 1; t <= T; ++t) {
        wave_lds_sync();
        float nv = 0.f;
#pragma unroll
        for (int j4 = 0; j4 < KP / 4; ++j4) {
            const f32x4 vv = *reinterpret_cast<const f32x4*>(&sh.V[t - 1][4 * j4]);
#pragma unroll
            for (int e = 0; e < 4; ++e) nv = fmaf(mrow[4 * j4 + e], vv[e], nv);
        }
        nv = valid ? nv : 0.f;
        const float nrm = sqrtf(wave_sum_dpp(nv * nv));
        v = nv / (nrm + 1e-6f);
        if (lane < KP) sh.V[t][lane] = v;
        if (lane == 0) sh.nrm[t] = nrm;
    }
    // ---- weighted Procrustes, forward (seed_procrustes of solver.hip)
    const float vsum = wave_sum_dpp(v) + 1e-6f;
    float w = v / vsum;
    const bool wlive = valid && !(w < 0.f);
    w = wlive ? w : 0.f;
    const float den = wave_sum_dpp(w) + 1e-6f;
    const float cA[3] = {wave_sum_dpp(ax * w) / den, wave_sum_dpp(ay * w) / den, wave_sum_dpp(az * w) / den};
    const float cB[3] = {wave_sum_dpp(bx * w) / den, wave_sum_dpp(by * w) / den, wave_sum_dpp(bz * w) / den};
    const float am[3] = {ax - cA[0], ay - cA[1], az - cA[2]};
    const float bm[3] = {bx - cB[0], by - cB[1], bz - cB[2]};
    double H[3][3], sA[3], sB[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int c = 0; c < 3; ++c) H[r][c] = (double)wave_sum_dpp(am[r] * w * bm[c]);
        sA[r] = (double)wave_sum_dpp(am[r] * w);
        sB[r] = (double)wave_sum_dpp(bm[r] * w);
    }
    // ---- the 3x3 part, fp64, every lane the same values
    double R[3][3], U[3][3], sp[3], gR[3][3], gt[3];
    ssb_kabsch(H, R, U, sp);
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        gt[r] = (double)__shfl(g, 4 * r + 3, 64);
#pragma unroll
        for (int c = 0; c < 3; ++c) gR[r][c] = (double)__shfl(g, 4 * r + c, 64) - gt[r] * (double)cA[c];      // t = cB - R cA
    }
    double Y[3][3], Z[3][3], Q[3][3], W1[3][3], gH[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) Y[i][j] = R[0][i] * gR[0][j] + R[1][i] * gR[1][j] + R[2][i] * gR[2][j];        // R^T gR
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) Z[i][j] = Y[i][j] - Y[j][i];
#pragma unroll
    for (int i = 0; i < 3; ++i)                                                                                  // W1 = Z U
#pragma unroll
        for (int j = 0; j < 3; ++j) W1[i][j] = Z[i][0] * U[0][j] + Z[i][1] * U[1][j] + Z[i][2] * U[2][j];
#pragma unroll
    for (int i = 0; i < 3; ++i)                                                                                  // Q = U^T Z U / (s'_i + s'_j)
#pragma unroll
        for (int j = 0; j < 3; ++j)
            Q[i][j] = i == j ? 0.0 : (U[0][i] * W1[0][j] + U[1][i] * W1[1][j] + U[2][i] * W1[2][j]) / (sp[i] + sp[j]);
#pragma unroll
    for (int i = 0; i < 3; ++i)                                                                                  // W1 = U Q
#pragma unroll
        for (int j = 0; j < 3; ++j) W1[i][j] = U[i][0] * Q[0][j] + U[i][1] * Q[1][j] + U[i][2] * Q[2][j];
#pragma unroll
    for (int i = 0; i < 3; ++i)                                                                                  // Z = U Q U^T
#pragma unroll
        for (int j = 0; j < 3; ++j) Z[i][j] = W1[i][0] * U[j][0] + W1[i][1] * U[j][1] + W1[i][2] * U[j][2];
#pragma unroll
    for (int i = 0; i < 3; ++i)                                                                                  // gH = (R U Q U^T)^T
#pragma unroll
        for (int j = 0; j < 3; ++j) gH[j][i] = R[i][0] * Z[0][j] + R[i][1] * Z[1][j] + R[i][2] * Z[2][j];
    float gHf[3][3], gcA[3], gcB[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const double ca = -(R[0][r] * gt[0] + R[1][r] * gt[1] + R[2][r] * gt[2]) - (gH[r][0] * sB[0] + gH[r][1] * sB[1] + gH[r][2] * sB[2]);
        const double cb = gt[r] - (gH[0][r] * sA[0] + gH[1][r] * sA[1] + gH[2][r] * sA[2]);
        gcA[r] = (float)ca; gcB[r] = (float)cb;
#pragma unroll
        for (int c = 0; c < 3; ++c) gHf[r][c] = (float)gH[r][c];
    }
    // ---- dw, dv_T
    float gw = 0.f;
#pragma unroll
    for (int r = 0; r < 3; ++r) gw += am[r] * ((gHf[r][0] * bm[0] + gHf[r][1] * bm[1]) + gHf[r][2] * bm[2]);
    gw += (((gcA[0] * am[0] + gcA[1] * am[1]) + gcA[2] * am[2]) + ((gcB[0] * bm[0] + gcB[1] * bm[1]) + gcB[2] * bm[2])) / den;
    gw = wlive ? gw : 0.f;
    float gv = (gw - wave_sum_dpp(gw * w)) / vsum;
    gv = valid ? gv : 0.f;
    // ---- the iterates backwards
    float dmrow[KP];
#pragma unroll
    for (int j = 0; j < KP; ++j) dmrow[j] = 0.f;
    for (int t = T; t >= 1; --t) {
        const float vt = lane < KP ? sh.V[t][lane] : 0.f;
        const float nrm = sh.nrm[t], e = nrm + 1e-6f;
        const float ut = vt * e;
        const float dot = wave_sum_dpp(gv * vt);
        float gu = (gv - dot * (ut / nrm)) / e;                   // nrm == 0: 0 / 0 = NaN, as autograd's
        gu = valid ? gu : 0.f;
        wave_lds_sync();                                          // the previous round's readers of sh.x are done
        if (lane < KP) sh.x[lane] = gu;
        wave_lds_sync();
        float ngv = 0.f;
#pragma unroll
        for (int j4 = 0; j4 < KP / 4; ++j4) {
            const f32x4 vp = *reinterpret_cast<const f32x4*>(&sh.V[t - 1][4 * j4]);
            const f32x4 xx = *reinterpret_cast<const f32x4*>(&sh.x[4 * j4]);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                dmrow[4 * j4 + q] = fmaf(gu, vp[q], dmrow[4 * j4 + q]);          // dM += du_t v_{t-1}^T
                ngv = fmaf(mrow[4 * j4 + q], xx[q], ngv);                        // dv_{t-1} = M^T du_t (M is symmetric bit for bit)
            }
        }
        gv = valid ? ngv : 0.f;
    }
    // ---- dM -> dMf (product, zero diagonal, clamp), the dsigma term
    wave_lds_sync();
    double dsg = 0.0;
#pragma unroll
    for (int j = 0; j < KP; ++j) {
        const f32x4 pj = *reinterpret_cast<const f32x4*>(&sh.pts[j][0]);
        const f32x4 qj = *reinterpret_cast<const f32x4*>(&sh.pts[j][4]);
        const float omg = sh.G[rowl * MLD + j];                                  // 1 - G_ij
        const float raw = 1.0f - omg * rsig2;
        const float sm = (float)ssb_spatial(ax, ay, az, bx, by, bz, pj, qj, sd2d);
        const bool live = valid && j < k && j != lane && raw >= 0.0f;            // inclusive: torch.clamp's backward
        const float dmf = live ? dmrow[j] * sm : 0.0f;
        dsg = fma((double)dmf, (double)omg, dsg);
        if (lane < KP) sh.M[lane * MLD + j] = dmf;
    }
    wave_lds_sync();
    if (lane < KP) {
#pragma unroll
        for (int j = 0; j < KP; ++j) sh.G[lane * MLD + j] = sh.M[lane * MLD + j] + sh.M[j * MLD + lane];
    }
    wave_lds_sync();
    // ---- dF_knn = (1 / sigma^2) (dMf + dMf^T) F_knn: lane = channels (lane, lane + 64), the k rows in registers
    float f0[KP], f1[KP];
#pragma unroll
    for (int j = 0; j < KP; ++j) {
        const int nbr = __shfl(idx, min(j, k - 1), 64);
        const float* row = nb + (size_t)nbr * PDSC_CHANNELS;
        f0[j] = row[lane];
        f1[j] = row[lane + 64];
    }
    const float nanv = __builtin_nanf("");
    float* blk = a.blocks + seed * (size_t)k * PDSC_CHANNELS;
    // (not vectorised over i: the loop vectoriser pairs two rows into v_pk_fma_f32 with operand selects, which the library does
    // not ship -- build.py, tools/isa_audit.py)
#pragma clang loop vectorize(disable) interleave(disable)
    for (int i = 0; i < k; ++i) {
        float a0 = 0.f, a1 = 0.f;
        const float* wr = sh.G + i * MLD;
#pragma unroll
        for (int j = 0; j < KP; ++j) {
            const float wij = wr[j];                              // (columns >= k are 0)
            a0 = fmaf(wij, f0[j], a0);
            a1 = fmaf(wij, f1[j], a1);
        }
        blk[(size_t)i * PDSC_CHANNELS + lane] = bad ? nanv : a0 * rsig2;
        blk[(size_t)i * PDSC_CHANNELS + lane + 64] = bad ? nanv : a1 * rsig2;
    }
    const double dsum = wave_sum(dsg);
    if (lane == 0) {
        const double s3 = (double)sg * (double)sg * (double)sg;
        a.part[seed] = bad ? (double)nanv : dsum * 2.0 / s3;
        a.active[seed] = 1;
    }
}

// owner pass: one wavefront per row of dnormed adds the rows of the seeds' blocks that name it, in (seed, neighbour) order
__global__ __launch_bounds__(256) void seed_solve_backward_owner_kernel(const int* __restrict__ knn_idx, const int* __restrict__ active,
                                                                        const float* __restrict__ blocks, float* __restrict__ dnormed,
                                                                        int N, int S, int k) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int row = blockIdx.x * 4 + wave, b = blockIdx.y;
    if (row >= N) return;                                         // wave-uniform; no barrier below
    float a0 = 0.f, a1 = 0.f;
    for (int s = 0; s < S; ++s) {
        const size_t seed = (size_t)b * S + s;
        if (!active[seed]) continue;                              // (uniform)
        const int id = lane < k ? knn_idx[seed * k + lane] : -1;
        unsigned long long m = __builtin_amdgcn_ballot_w64(id == row);
        while (m) {
            const int j = __builtin_ctzll(m);
            m &= m - 1;
            const float* p = blocks + (seed * k + j) * PDSC_CHANNELS;
            a0 += p[lane];
            a1 += p[lane + 64];
        }
    }
    float* d = dnormed + ((size_t)b * N + row) * PDSC_CHANNELS;
    d[lane] = a0;
    d[lane + 64] = a1;
}

// dsigma = the active seeds' terms: lane l adds seeds l, l + 64, ... in order, then the shuffle tree
__global__ __launch_bounds__(64) void seed_solve_backward_finish_kernel(const double* __restrict__ part, const int* __restrict__ active,
                                                                        int count, double* __restrict__ dsigma) {
    double d = 0.0;
    for (int p = threadIdx.x; p < count; p += 64)
        if (active[p]) d += part[p];
    d = wave_sum(d);
    if (threadIdx.x == 0) dsigma[0] = d;
}

static size_t ssb_blocks_bytes(int bs, int S, int k) { return (size_t)bs * S * k * PDSC_CHANNELS * sizeof(float); }

}  // namespace pdsc

extern "C" size_t pdsc_seed_solve_backward_workspace_bytes(int bs, int N, int S, int k) {
    if (bs <= 0 || N <= 0 || S <= 0 || k < 1 || k > PDSC_MAX_K) return 0;
    return pdsc::ssb_blocks_bytes(bs, S, k) + (size_t)bs * S * (sizeof(double) + sizeof(int));
}

extern "C" int pdsc_seed_solve_backward(const float* normed, const float* src, const float* tgt, const int* knn_idx, const float* sigma,
                                        const float* sigma_spat, const unsigned int* conv_mask, const float* d_seed_trans, float* dnormed,
                                        double* dsigma, void* ws, size_t ws_bytes, int bs, int N, int S, int k, int num_iterations,
                                        void* stream) {
    PDSC_REQUIRE(normed && src && tgt && knn_idx && sigma && sigma_spat && conv_mask && d_seed_trans, "pdsc_seed_solve_backward: null pointer");
    PDSC_REQUIRE(dnormed || dsigma, "pdsc_seed_solve_backward: neither gradient asked for");
    PDSC_REQUIRE(bs > 0 && N > 0 && S > 0 && bs <= 65535, "pdsc_seed_solve_backward: bs=%d N=%d S=%d", bs, N, S);
    PDSC_REQUIRE(k >= 1 && k <= PDSC_MAX_K, "pdsc_seed_solve_backward: k=%d (max %d)", k, PDSC_MAX_K);
    PDSC_REQUIRE(num_iterations >= 0 && num_iterations <= PDSC_MAX_POWER_ITERS, "pdsc_seed_solve_backward: num_iterations=%d (max %d)",
                 num_iterations, PDSC_MAX_POWER_ITERS);
    PDSC_REQUIRE(((uintptr_t)normed & 15) == 0, "pdsc_seed_solve_backward: normed must be 16-byte aligned");
    PDSC_REQUIRE(ws && ((uintptr_t)ws & 7) == 0, "pdsc_seed_solve_backward: workspace must be 8-byte aligned");
    if (ws_bytes < pdsc_seed_solve_backward_workspace_bytes(bs, N, S, k)) {
        pdsc::set_error("pdsc_seed_solve_backward: workspace of %zu bytes, needs %zu", ws_bytes,
                        pdsc_seed_solve_backward_workspace_bytes(bs, N, S, k));
        return PDSC_ERR_WORKSPACE;
    }
    hipStream_t st = (hipStream_t)stream;
    pdsc::SsbArgs a{};
    a.normed = normed; a.src = src; a.tgt = tgt; a.knn_idx = knn_idx; a.sigma = sigma; a.sigma_spat = sigma_spat;
    a.conv_mask = conv_mask; a.dtrans = d_seed_trans;
    a.blocks = (float*)ws;
    a.part = (double*)((char*)ws + pdsc::ssb_blocks_bytes(bs, S, k));
    a.active = (int*)(a.part + (size_t)bs * S);
    a.N = N; a.S = S; a.k = k; a.num_iter = num_iterations;
    const int nb = pdsc::ceil_div(k, 16);
    const dim3 grid(S, bs);
    if (nb == 1) hipLaunchKernelGGL(pdsc::seed_solve_backward_kernel<1>, grid, dim3(64), 0, st, a);
    else if (nb == 2) hipLaunchKernelGGL(pdsc::seed_solve_backward_kernel<2>, grid, dim3(64), 0, st, a);
    else if (nb == 3) hipLaunchKernelGGL(pdsc::seed_solve_backward_kernel<3>, grid, dim3(64), 0, st, a);
    else hipLaunchKernelGGL(pdsc::seed_solve_backward_kernel<4>, grid, dim3(64), 0, st, a);
    int rc = pdsc::check_launch("pdsc_seed_solve_backward");
    if (rc != PDSC_OK) return rc;
    if (dnormed)
        hipLaunchKernelGGL(pdsc::seed_solve_backward_owner_kernel, dim3(pdsc::ceil_div(N, 4), bs), dim3(256), 0, st, knn_idx, a.active,
                           a.blocks, dnormed, N, S, k);
    if (dsigma)
        hipLaunchKernelGGL(pdsc::seed_solve_backward_finish_kernel, dim3(1), dim3(64), 0, st, a.part, a.active, bs * S, dsigma);
    return pdsc::check_launch("pdsc_seed_solve_backward(owner pass)");
}
