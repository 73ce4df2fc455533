// The 3x3 fp64 core of the library (DESIGN.md "3x3 SVD"): the cyclic Jacobi eigen-decomposition of a symmetric 3x3 matrix, once, and
// the one Kabsch solve built on it -- the forward's fp32 entry, ICP's fp64 entry and the entry of the seed-solve backward, which
// differentiates the decomposition the forward chose and therefore has to take exactly its branches (sweep exit, eigenvalue order,
// the rank <= 1 fallback).  Included by pdsc_common.h alone, inside namespace pdsc and after <math.h>: include that file.
#pragma once
#ifndef PDSC_COMMON_INCLUDES_KABSCH3
#error "kabsch3.h is a part of pdsc_common.h (it sits inside namespace pdsc): include pdsc_common.h"
#endif

// Cyclic Jacobi on the symmetric A (fp64, at most SWEEPS sweeps; stops when the off-diagonal sum is <= tol * the diagonal sum):
// on return the diagonal of A holds the eigenvalues and the columns of V the eigenvectors, in no particular order.
template <int SWEEPS>
__device__ __forceinline__ void jacobi_eig3(double (&A)[3][3], double (&V)[3][3], const double tol) {
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) V[i][j] = i == j ? 1.0 : 0.0;
    for (int sweep = 0; sweep < SWEEPS; ++sweep) {
        const double off = fabs(A[0][1]) + fabs(A[0][2]) + fabs(A[1][2]);
        const double diag = fabs(A[0][0]) + fabs(A[1][1]) + fabs(A[2][2]);
        if (off <= 1e-300 || off <= tol * diag) break;
#pragma unroll
        for (int pq = 0; pq < 3; ++pq) {
            const int p = (pq == 2) ? 1 : 0;
            const int q = (pq == 0) ? 1 : 2;
            const double apq = A[p][q];
            if (fabs(apq) < 1e-300) continue;
            const double theta = (A[q][q] - A[p][p]) / (2.0 * apq);
            const double tt = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
            const double c = 1.0 / sqrt(tt * tt + 1.0), s = tt * c;
#pragma unroll
            for (int r = 0; r < 3; ++r) {  // A <- A J
                const double arp = A[r][p], arq = A[r][q];
                A[r][p] = c * arp - s * arq;
                A[r][q] = s * arp + c * arq;
            }
#pragma unroll
            for (int r = 0; r < 3; ++r) {  // A <- J^T A
                const double apr = A[p][r], aqr = A[q][r];
                A[p][r] = c * apr - s * aqr;
                A[q][r] = s * apr + c * aqr;
            }
#pragma unroll
            for (int r = 0; r < 3; ++r) {  // V <- V J
                const double vrp = V[r][p], vrq = V[r][q];
                V[r][p] = c * vrp - s * vrq;
                V[r][q] = s * vrp + c * vrq;
            }
        }
    }
}

// ---- Kabsch from a 3x3 weighted covariance -----------------------------------------------------
// reference models/common.py:35-42: U,S,V = svd(H); R = V diag(1,1,det(V U^T)) U^T; t = cB - R cA.
// Computed as: eigen-decomposition of H^T H (cyclic Jacobi, fp64) -> V, sigma; u_i = H v_i / sigma_i for the
// two leading directions, u_3 = u_1 x u_2 (so det U = +1), which yields the same R whenever rank(H) >= 2.
// Hin row-major (H[r][c] = sum a_r b_c) and the centroids of type TI; FACTORS = false: T, row-major 4x4 of type TO with t = cB - R cA;
// FACTORS = true (the backward; cA, cB, T unused): R and U = (u1 u2 u3) as columns, row-major fp64, and s' = (s1, s2, u3 . H v3).
// One function and not smaller pieces: with R, U, s' handed between pieces as arrays the forward's kernels grew (VGPRs
// kabsch_batch / fixup_kabsch 88 -> 109, rigid_transform 74 -> 84, refine / select_refine 99 -> 106); as one body they keep 88 / 74 / 99.
template <typename TI, typename TO, bool FACTORS>
__device__ inline void kabsch3(const TI* Hin, const TI* cA, const TI* cB, TO* T, double* Rout, double* Uout, double* sp) {
    double H[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) H[i][j] = (double)Hin[i * 3 + j];
    // A = H^T H (symmetric)
    double A[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) A[i][j] = H[0][i] * H[0][j] + H[1][i] * H[1][j] + H[2][i] * H[2][j];
    double V[3][3];
    jacobi_eig3<12>(A, V, 1e-17);
    // order eigenvalues descending: i0 >= i1 >= i2
    int i0 = 0, i1 = 1, i2 = 2;
    double e0 = A[0][0], e1 = A[1][1], e2 = A[2][2];
    if (e0 < e1) { double t = e0; e0 = e1; e1 = t; int ti = i0; i0 = i1; i1 = ti; }
    if (e0 < e2) { double t = e0; e0 = e2; e2 = t; int ti = i0; i0 = i2; i2 = ti; }
    if (e1 < e2) { double t = e1; e1 = e2; e2 = t; int ti = i1; i1 = i2; i2 = ti; }
    (void)i2;
    // select columns with compares (runtime-indexed local arrays would go to scratch memory)
#define PDSC_SEL3(r, i) ((i) == 0 ? V[r][0] : ((i) == 1 ? V[r][1] : V[r][2]))
    double v1[3] = {PDSC_SEL3(0, i0), PDSC_SEL3(1, i0), PDSC_SEL3(2, i0)};
    double v2[3] = {PDSC_SEL3(0, i1), PDSC_SEL3(1, i1), PDSC_SEL3(2, i1)};
#undef PDSC_SEL3
    // v3 = v1 x v2 makes (v1,v2,v3) right-handed; the sign of v3 is irrelevant below because it enters
    // R only through d * v3 u3^T with d = det(V) det(U) and u3 = u1 x u2 (det U = +1).
    double v3[3] = {v1[1] * v2[2] - v1[2] * v2[1], v1[2] * v2[0] - v1[0] * v2[2], v1[0] * v2[1] - v1[1] * v2[0]};
    // u1 = H v1 / |H v1|
    double u1[3], u2[3], u3[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) u1[i] = H[i][0] * v1[0] + H[i][1] * v1[1] + H[i][2] * v1[2];
    double n1 = sqrt(u1[0] * u1[0] + u1[1] * u1[1] + u1[2] * u1[2]);
    if (n1 > 1e-150) { u1[0] /= n1; u1[1] /= n1; u1[2] /= n1; }
    else { u1[0] = 1; u1[1] = 0; u1[2] = 0; }              // H == 0: any basis (R not defined by H)
#pragma unroll
    for (int i = 0; i < 3; ++i) u2[i] = H[i][0] * v2[0] + H[i][1] * v2[1] + H[i][2] * v2[2];
    double dp = u2[0] * u1[0] + u2[1] * u1[1] + u2[2] * u1[2];
    u2[0] -= dp * u1[0]; u2[1] -= dp * u1[1]; u2[2] -= dp * u1[2];
    double n2 = sqrt(u2[0] * u2[0] + u2[1] * u2[1] + u2[2] * u2[2]);
    if (n2 > 1e-12 * (n1 > 1e-150 ? n1 : 1.0) && n2 > 1e-150) { u2[0] /= n2; u2[1] /= n2; u2[2] /= n2; }
    else {  // rank <= 1: pick any unit vector orthogonal to u1
        int m = (fabs(u1[0]) <= fabs(u1[1]) && fabs(u1[0]) <= fabs(u1[2])) ? 0 : (fabs(u1[1]) <= fabs(u1[2]) ? 1 : 2);
        const double e[3] = {m == 0 ? 1.0 : 0.0, m == 1 ? 1.0 : 0.0, m == 2 ? 1.0 : 0.0};
        double d2 = e[0] * u1[0] + e[1] * u1[1] + e[2] * u1[2];
        u2[0] = e[0] - d2 * u1[0]; u2[1] = e[1] - d2 * u1[1]; u2[2] = e[2] - d2 * u1[2];
        n2 = sqrt(u2[0] * u2[0] + u2[1] * u2[1] + u2[2] * u2[2]);
        u2[0] /= n2; u2[1] /= n2; u2[2] /= n2;
        if constexpr (FACTORS) n2 = 0.0;                     // rank <= 1: the second singular value
    }
    u3[0] = u1[1] * u2[2] - u1[2] * u2[1];
    u3[1] = u1[2] * u2[0] - u1[0] * u2[2];
    u3[2] = u1[0] * u2[1] - u1[1] * u2[0];
    // with v3 = v1 x v2 and u3 = u1 x u2 both bases are right-handed: det(V) det(U) = +1, so
    // R = v1 u1^T + v2 u2^T + v3 u3^T is the proper rotation the reference's det-correction selects.
    double R[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) R[i][j] = v1[i] * u1[j] + v2[i] * u2[j] + v3[i] * u3[j];
    if constexpr (FACTORS) {
        double hv3[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) hv3[i] = H[i][0] * v3[0] + H[i][1] * v3[1] + H[i][2] * v3[2];
        sp[0] = n1; sp[1] = n2; sp[2] = u3[0] * hv3[0] + u3[1] * hv3[1] + u3[2] * hv3[2];      // signed: det(V U^T) s3
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            Uout[i * 3 + 0] = u1[i]; Uout[i * 3 + 1] = u2[i]; Uout[i * 3 + 2] = u3[i];
#pragma unroll
            for (int j = 0; j < 3; ++j) Rout[i * 3 + j] = R[i][j];
        }
    } else {
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const double ti = (double)cB[i] - (R[i][0] * (double)cA[0] + R[i][1] * (double)cA[1] + R[i][2] * (double)cA[2]);
            T[i * 4 + 0] = (TO)R[i][0];
            T[i * 4 + 1] = (TO)R[i][1];
            T[i * 4 + 2] = (TO)R[i][2];
            T[i * 4 + 3] = (TO)ti;
        }
        T[12] = (TO)0; T[13] = (TO)0; T[14] = (TO)0; T[15] = (TO)1;
    }
}

// the forward (kabsch_batch_kernel, fixup_kabsch_kernel, rigid_transform_kernel, refine_kernel / select_refine_kernel): fp32 in and out
__device__ inline void kabsch_from_covariance(const float* H32, const float* cA, const float* cB, float* T) {
    kabsch3<float, float, false>(H32, cA, cB, T, nullptr, nullptr, nullptr);
}
// ICP (Eigen's umeyama without scaling): covariance, centroids and pose fp64
__device__ inline void kabsch_from_covariance_f64(const double* H64, const double* cA, const double* cB, double* T) {
    kabsch3<double, double, false>(H64, cA, cB, T, nullptr, nullptr, nullptr);
}
// the seed-solve backward: the forward's solve of H, returning what its adjoint needs (R, U, s')
__device__ inline void ssb_kabsch(const double (&H)[3][3], double (&R)[3][3], double (&U)[3][3], double (&sp)[3]) {
    kabsch3<double, double, true>(&H[0][0], nullptr, nullptr, nullptr, &R[0][0], &U[0][0], sp);
}
