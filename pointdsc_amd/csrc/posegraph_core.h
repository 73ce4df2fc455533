// f-8: pose-graph optimisation (open3d 0.9 GlobalOptimization with GlobalOptimizationLevenbergMarquardt, restated in DESIGN.md
// section 8 f-8 and in include/pointdsc_hip.h).  Everything here is __host__ __device__ and written against a "team": `tid` of `nt`
// cooperating threads with sync() / sum() / maxv() / any() / clock().  On the device the team is one 512-thread workgroup (posegraph.hip); on
// the host a team of one thread runs the very same code sequentially -- every phase between two sync() calls is data-parallel, so
// the sequential run computes the same thing (sums in another order) and can be compared with the fp64 oracle without a GPU.
// All index arithmetic of local arrays is static (fully unrolled loops): nothing here may end up in scratch memory.
#pragma once
#include <float.h>
#include <math.h>

#if defined(__HIPCC__)
#define PG_HD __host__ __device__ __forceinline__
#else
#define PG_HD inline
#endif

namespace pdsc {
namespace pg {

constexpr int NB = 16;          // Cholesky block width
constexpr int LD = NB + 1;      // row stride of the LDS panels (odd: rows fall into different banks)
constexpr int EM = 42;          // per-edge record: Js^T Lambda Js [36] | Js^T Lambda e [6]
constexpr int REC = 12;         // PDSC_POSEGRAPH_RECORD

PG_HD bool finite_d(double v) { return fabs(v) <= DBL_MAX; }

// C = A B, all row-major 4x4; every entry ((a0 b0 + a1 b1) + a2 b2) + a3 b3
PG_HD void mul44(const double* A, const double* B, double* C) {
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c)
            C[r * 4 + c] = ((A[r * 4] * B[c] + A[r * 4 + 1] * B[4 + c]) + A[r * 4 + 2] * B[8 + c]) + A[r * 4 + 3] * B[12 + c];
}

// INVERSE_RULE: [R^-1, -R^-1 t; 0 0 0 1] with R^-1 = adj(R) / det(R) (not R^T)
PG_HD void inv_rigid(const double* T, double* O) {
    const double a = T[0], b = T[1], c = T[2], d = T[4], e = T[5], f = T[6], g = T[8], h = T[9], i = T[10];
    const double c00 = e * i - f * h, c10 = f * g - d * i, c20 = d * h - e * g;
    const double det = (a * c00 + b * c10) + c * c20;
    O[0] = c00 / det; O[1] = (c * h - b * i) / det; O[2] = (b * f - c * e) / det;
    O[4] = c10 / det; O[5] = (a * i - c * g) / det; O[6] = (c * d - a * f) / det;
    O[8] = c20 / det; O[9] = (b * g - a * h) / det; O[10] = (a * e - b * d) / det;
    O[3] = -((O[0] * T[3] + O[1] * T[7]) + O[2] * T[11]);
    O[7] = -((O[4] * T[3] + O[5] * T[7]) + O[6] * T[11]);
    O[11] = -((O[8] * T[3] + O[9] * T[7]) + O[10] * T[11]);
    O[12] = 0.0; O[13] = 0.0; O[14] = 0.0; O[15] = 1.0;
}

// vec2mat: R = Rz(v2) Ry(v1) Rx(v0), t = v[3:6]
PG_HD void vec2mat(const double* v, double* T) {
    const double sx = sin(v[0]), cx = cos(v[0]), sy = sin(v[1]), cy = cos(v[1]), sz = sin(v[2]), cz = cos(v[2]);
    T[0] = cz * cy; T[1] = (cz * sy) * sx - sz * cx; T[2] = (cz * sy) * cx + sz * sx; T[3] = v[3];
    T[4] = sz * cy; T[5] = (sz * sy) * sx + cz * cx; T[6] = (sz * sy) * cx - cz * sx; T[7] = v[4];
    T[8] = -sy;     T[9] = cy * sx;                  T[10] = cy * cx;                 T[11] = v[5];
    T[12] = 0.0; T[13] = 0.0; T[14] = 0.0; T[15] = 1.0;
}

// mat2vec (used only for |x|)
PG_HD void mat2vec(const double* T, double* v) {
    const double sy = hypot(T[0], T[4]);
    if (!(sy < 1e-6)) {
        v[0] = atan2(T[9], T[10]); v[1] = atan2(-T[8], sy); v[2] = atan2(T[4], T[0]);
    } else {
        v[0] = atan2(-T[6], T[5]); v[1] = atan2(-T[8], sy); v[2] = 0.0;
    }
    v[3] = T[3]; v[4] = T[7]; v[5] = T[11];
}

// lin6 of N = A G P for a rotation generator G with G[V][U] = 1, G[U][V] = -1 ... written out: N[r][c] = A[r][U] P[P_][c] - A[r][V] P[Q][c]
template <int U, int P_, int V, int Q>
PG_HD void jac_rot(const double* A, const double* P, double* Js, int k) {
#define PG_N(r, c) (A[(r) * 4 + U] * P[P_ * 4 + (c)] - A[(r) * 4 + V] * P[Q * 4 + (c)])
    Js[0 * 6 + k] = (PG_N(2, 1) - PG_N(1, 2)) / 2.0;
    Js[1 * 6 + k] = (PG_N(0, 2) - PG_N(2, 0)) / 2.0;
    Js[2 * 6 + k] = (PG_N(1, 0) - PG_N(0, 1)) / 2.0;
    Js[3 * 6 + k] = PG_N(0, 3);
    Js[4 * 6 + k] = PG_N(1, 3);
    Js[5 * 6 + k] = PG_N(2, 3);
#undef PG_N
}
// translation generator G[U][3] = 1: N[r][c] = A[r][U] P[3][c]
template <int U>
PG_HD void jac_trans(const double* A, const double* P, double* Js, int k) {
#define PG_N(r, c) (A[(r) * 4 + U] * P[12 + (c)])
    Js[0 * 6 + k] = (PG_N(2, 1) - PG_N(1, 2)) / 2.0;
    Js[1 * 6 + k] = (PG_N(0, 2) - PG_N(2, 0)) / 2.0;
    Js[2 * 6 + k] = (PG_N(1, 0) - PG_N(0, 1)) / 2.0;
    Js[3 * 6 + k] = PG_N(0, 3);
    Js[4 * 6 + k] = PG_N(1, 3);
    Js[5 * 6 + k] = PG_N(2, 3);
#undef PG_N
}

// One edge: A = X^-1 pose_t^-1, e = lin6(A pose_s), q = e^T Lambda e and (Js != NULL) Js[a][k] = lin6(A G_k pose_s)[a].
PG_HD void edge_eval(const double* X, const double* Ps, const double* Pt, const double* Lam, double* e_out, double* q_out, double* Js) {
    double x[16], ps[16], pt[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) { x[k] = X[k]; ps[k] = Ps[k]; pt[k] = Pt[k]; }
    double Xi[16], Ti[16], A[16], M[16];
    inv_rigid(x, Xi);
    inv_rigid(pt, Ti);
    mul44(Xi, Ti, A);
    mul44(A, ps, M);
    double e[6];
    e[0] = (M[9] - M[6]) / 2.0; e[1] = (M[2] - M[8]) / 2.0; e[2] = (M[4] - M[1]) / 2.0;
    e[3] = M[3]; e[4] = M[7]; e[5] = M[11];
    double q = 0.0;
#pragma unroll
    for (int a = 0; a < 6; ++a) {
        double s = 0.0;
#pragma unroll
        for (int b = 0; b < 6; ++b) s += Lam[a * 6 + b] * e[b];
        q += e[a] * s;
    }
#pragma unroll
    for (int a = 0; a < 6; ++a) e_out[a] = e[a];
    *q_out = q;
    if (Js) {
        jac_rot<2, 1, 1, 2>(A, ps, Js, 0);      // alpha: G[1][2] = -1, G[2][1] = 1
        jac_rot<0, 2, 2, 0>(A, ps, Js, 1);      // beta:  G[0][2] = 1,  G[2][0] = -1
        jac_rot<1, 0, 0, 1>(A, ps, Js, 2);      // gamma: G[0][1] = -1, G[1][0] = 1
        jac_trans<0>(A, ps, Js, 3);
        jac_trans<1>(A, ps, Js, 4);
        jac_trans<2>(A, ps, Js, 5);
    }
}

// Row r of Js^T Lambda Js and entry r of Js^T Lambda e: v = (Js^T Lambda)[r][:], then v Js and v e.
PG_HD void edge_normal_row(const double* Js, const double* Lam, const double* e, int r, double* out_row, double* out_g) {
    double v[6];
#pragma unroll
    for (int b = 0; b < 6; ++b) {
        double s = 0.0;
#pragma unroll
        for (int a = 0; a < 6; ++a) s += Js[a * 6 + r] * Lam[a * 6 + b];
        v[b] = s;
    }
    double g = 0.0;
#pragma unroll
    for (int b = 0; b < 6; ++b) g += v[b] * e[b];
    *out_g = g;
#pragma unroll
    for (int c = 0; c < 6; ++c) {
        double s = 0.0;
#pragma unroll
        for (int b = 0; b < 6; ++b) s += v[b] * Js[b * 6 + c];
        out_row[c] = s;
    }
}

// ---- (H + lam I) delta = b: blocked in-place Cholesky with the right-hand side as one more row ---------------------------
// L is (n + 1) x n, row-major with stride n: rows 0..n-1 := H + lam I (lower triangle is what counts), row n := b.  The
// factorisation runs over the n columns and all n + 1 rows, so that row n leaves as y = L^-1 b (the forward substitution is
// the panel solve of that row); the blocked back substitution L^T delta = y follows.  Per block column of NB: the diagonal
// block is factored in `dblk` (NB x LD), the rows below are solved against it into `panel` ((n + 1) x LD), then every thread
// updates 4 x 4 tiles of the trailing matrix from the panel.  Every entry is computed by one thread in a fixed order of
// operations (there is no cross-thread sum), so the bits do not depend on the size of the team.
template <class Team>
PG_HD void solve_spd(const double* H, const double* b, double lam, int n, double* L, double* delta, double* panel, double* dblk,
                     const Team& tm) {
    for (int idx = tm.tid; idx < n * n; idx += tm.nt) {
        const int i = idx / n, j = idx - i * n;
        L[idx] = i == j ? H[idx] + lam : H[idx];
    }
    for (int j = tm.tid; j < n; j += tm.nt) L[n * n + j] = b[j];
    tm.sync();
    const int rows = n + 1;
    for (int k0 = 0; k0 < n; k0 += NB) {
        const int nb = n - k0 < NB ? n - k0 : NB;
        for (int idx = tm.tid; idx < NB * NB; idx += tm.nt) {
            const int r = idx / NB, c = idx % NB;
            if (r < nb && c <= r) dblk[r * LD + c] = L[(k0 + r) * n + k0 + c];
        }
        tm.sync();
        // right-looking inside the block; column j stays unscaled (a_rj of step j) until the end
        for (int j = 0; j < nb; ++j) {
            for (int idx = tm.tid; idx < NB * NB; idx += tm.nt) {
                const int r = idx / NB, c = idx % NB;
                if (r < nb && c > j && c <= r) {
                    const double d = sqrt(dblk[j * LD + j]);
                    dblk[r * LD + c] = fma(-(dblk[r * LD + j] / d), dblk[c * LD + j] / d, dblk[r * LD + c]);
                }
            }
            tm.sync();
        }
        for (int idx = tm.tid; idx < NB * NB; idx += tm.nt) {
            const int r = idx / NB, c = idx % NB;
            if (r < nb && c < r) dblk[r * LD + c] /= sqrt(dblk[c * LD + c]);
        }
        tm.sync();
        for (int r = tm.tid; r < nb; r += tm.nt) dblk[r * LD + r] = sqrt(dblk[r * LD + r]);
        tm.sync();
        for (int idx = tm.tid; idx < NB * NB; idx += tm.nt) {
            const int r = idx / NB, c = idx % NB;
            if (r < nb && c <= r) L[(k0 + r) * n + k0 + c] = dblk[r * LD + c];
        }
        // panel: rows below the block (the right-hand side row included) times the inverse transpose of the block
        const int base = k0 + nb, m = rows - base;
        for (int ri = tm.tid; ri < m; ri += tm.nt) {
            double* row = L + (size_t)(base + ri) * n + k0;
            for (int j = 0; j < nb; ++j) {
                double s = row[j];
                for (int p = 0; p < j; ++p) s = fma(-panel[ri * LD + p], dblk[j * LD + p], s);
                s /= dblk[j * LD + j];
                panel[ri * LD + j] = s;
                row[j] = s;
            }
        }
        tm.sync();
        // trailing update, lower triangle, 4 x 4 tiles (ti >= tj)
        const int mt = (m + 3) / 4, ntile = mt * (mt + 1) / 2;
        for (int idx = tm.tid; idx < ntile; idx += tm.nt) {
            int ti = (int)((sqrt(8.0 * (double)idx + 1.0) - 1.0) * 0.5);
            while (ti * (ti + 1) / 2 > idx) --ti;
            while ((ti + 1) * (ti + 2) / 2 <= idx) ++ti;
            const int tj = idx - ti * (ti + 1) / 2;
            int ia[4], ja[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                ia[r] = ti * 4 + r < m ? ti * 4 + r : m - 1;
                ja[r] = tj * 4 + r < m ? tj * 4 + r : m - 1;
            }
            double acc[4][4];
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int c = 0; c < 4; ++c) acc[r][c] = 0.0;
            for (int p = 0; p < nb; ++p) {
                double av[4], bv[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) { av[r] = panel[ia[r] * LD + p]; bv[r] = panel[ja[r] * LD + p]; }
#pragma unroll
                for (int r = 0; r < 4; ++r)
#pragma unroll
                    for (int c = 0; c < 4; ++c) acc[r][c] = fma(av[r], bv[c], acc[r][c]);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const int i = ti * 4 + r, j = tj * 4 + c;
                    if (i < m && j <= i && base + j < n) L[(size_t)(base + i) * n + base + j] -= acc[r][c];
                }
        }
        tm.sync();
    }
    // L^T delta = y, block columns from the right
    for (int j = tm.tid; j < n; j += tm.nt) delta[j] = L[n * n + j];
    tm.sync();
    for (int k0 = ((n - 1) / NB) * NB; k0 >= 0; k0 -= NB) {
        const int nb = n - k0 < NB ? n - k0 : NB;
        for (int idx = tm.tid; idx < NB * NB; idx += tm.nt) {
            const int r = idx / NB, c = idx % NB;
            if (r < nb && c <= r) dblk[r * LD + c] = L[(k0 + r) * n + k0 + c];
        }
        for (int j = tm.tid; j < nb; j += tm.nt) panel[j] = delta[k0 + j];
        tm.sync();
        if (tm.tid == 0) {
            for (int j = nb - 1; j >= 0; --j) {
                double s = panel[j];
                for (int p = j + 1; p < nb; ++p) s = fma(-dblk[p * LD + j], panel[p], s);
                s /= dblk[j * LD + j];
                panel[j] = s;
                delta[k0 + j] = s;
            }
        }
        tm.sync();
        for (int j = tm.tid; j < k0; j += tm.nt) {
            double s = delta[j];
            for (int p = 0; p < nb; ++p) s = fma(-L[(size_t)(k0 + p) * n + j], panel[p], s);
            delta[j] = s;
        }
        tm.sync();
    }
}

// ---- one graph -------------------------------------------------------------------------------------------------------------------
struct Graph {
    int F, E;
    const double* nodes_in;             // [F][16]
    const int* src;                     // [E], graph-local node index
    const int* tgt;
    const double* X;                    // [E][16]
    const double* info;                 // [E][36]
    const unsigned char* uncertain;     // [E]
    const unsigned char* live_in;       // [E] or NULL
    double* nodes_out;                  // [F][16]
    double* conf;                       // [E]
    unsigned char* live;                // [E] (the output mask is the working mask)
    double* rec;                        // [REC]
    long long* ticks;                   // [3] or NULL: team clock ticks in residuals + assembly, in solves, in the whole graph
    // workspace (global memory)
    double *H, *L, *b, *delta, *poses, *trial, *zeta, *q, *Js, *em;
    int *inc_start, *inc;
    int* lidx;                          // [E + 1]: the live edges in ascending index, then their number (rebuilt per pass)
    // panels (LDS on the device)
    double *panel, *dblk;
    double max_distance, prune_threshold, preference;
    int reference;
};

template <class Team>
PG_HD void evaluate_edges(const Graph& g, const double* P, bool with_jacobian, const Team& tm) {
    for (int j = tm.tid; j < g.lidx[g.E]; j += tm.nt) {
        const int e = g.lidx[j];
        edge_eval(g.X + (size_t)e * 16, P + (size_t)g.src[e] * 16, P + (size_t)g.tgt[e] * 16, g.info + (size_t)e * 36, g.zeta + (size_t)e * 6,
                  g.q + e, with_jacobian ? g.Js + (size_t)e * 36 : nullptr);
    }
    tm.sync();
}

// sum over the live edges (in list order) of l q + w (sqrt(l) - 1)^2 (uncertain) or q (certain)
template <class Team>
PG_HD double objective(const Graph& g, double w, const Team& tm) {
    double v = 0.0;
    for (int j = tm.tid; j < g.lidx[g.E]; j += tm.nt) {
        const int e = g.lidx[j];
        if (g.uncertain[e]) {
            const double l = g.conf[e], r = sqrt(l) - 1.0;
            v += l * g.q[e] + w * (r * r);
        } else {
            v += g.q[e];
        }
    }
    return tm.sum(v);
}

template <class Team>
PG_HD void update_confidence(const Graph& g, double w, const Team& tm) {
    for (int j = tm.tid; j < g.lidx[g.E]; j += tm.nt) {
        const int e = g.lidx[j];
        if (!g.uncertain[e]) continue;
        const double r = w / (w + g.q[e]);
        g.conf[e] = r * r;
    }
    tm.sync();
}

// H and b from zeta / Js at the current poses: per-edge normal blocks, then every (node, entry) sums its incident edges in ascending
// edge index (one thread owns block row i, entry k, for all block columns: no two threads ever write the same word).
template <class Team>
PG_HD void build_system(const Graph& g, const Team& tm) {
    const int n = 6 * g.F;
    for (int idx = tm.tid; idx < 6 * g.lidx[g.E]; idx += tm.nt) {
        const int e = g.lidx[idx / 6], r = idx % 6;
        edge_normal_row(g.Js + (size_t)e * 36, g.info + (size_t)e * 36, g.zeta + (size_t)e * 6, r, g.em + (size_t)e * EM + r * 6,
                        g.em + (size_t)e * EM + 36 + r);
    }
    for (int idx = tm.tid; idx < n * n; idx += tm.nt) g.H[idx] = 0.0;
    tm.sync();
    for (int idx = tm.tid; idx < g.F * EM; idx += tm.nt) {
        const int i = idx / EM, k = idx - i * EM;
        const int r = k < 36 ? k / 6 : k - 36, c = k < 36 ? k - (k / 6) * 6 : 0;
        double acc = 0.0;
        for (int jj = g.inc_start[i]; jj < g.inc_start[i + 1]; ++jj) {
            const int e = g.inc[jj];
            if (!g.live[e]) continue;
            const double l = g.uncertain[e] ? g.conf[e] : 1.0;
            const double v = l * g.em[(size_t)e * EM + k];
            const int s = g.src[e];
            if (k < 36) {
                const int other = s == i ? g.tgt[e] : s;
                acc += v;                                                  // H[i][i] += l Js^T Lambda Js (Jt = -Js: the same block)
                g.H[(size_t)(6 * i + r) * n + 6 * other + c] -= v;         // H[i][other] += l Js^T Lambda Jt = -(l Js^T Lambda Js)
            } else {
                acc = s == i ? acc - v : acc + v;                          // b[s] -= l Js^T Lambda e;  b[t] -= l Jt^T Lambda e
            }
        }
        if (k < 36) g.H[(size_t)(6 * i + r) * n + 6 * i + c] = acc;
        else g.b[6 * i + r] = acc;
    }
    tm.sync();
}

template <class Team>
PG_HD double pose_vector_norm(const Graph& g, const double* P, const Team& tm) {
    double v = 0.0;
    for (int i = tm.tid; i < g.F; i += tm.nt) {
        double T[16], x[6];
#pragma unroll
        for (int k = 0; k < 16; ++k) T[k] = P[(size_t)i * 16 + k];
        mat2vec(T, x);
#pragma unroll
        for (int k = 0; k < 6; ++k) v += x[k] * x[k];
    }
    return sqrt(tm.sum(v));
}

template <class Team>
PG_HD double max_of(const double* v, int count, int stride, const Team& tm) {
    double m = -DBL_MAX;
    for (int i = tm.tid; i < count; i += tm.nt) m = fmax(m, v[(size_t)i * stride]);
    return tm.maxv(m);
}

// One optimisation pass (steps 1 - 11 of the contract) on the live edges; poses in g.poses on entry and on exit.
template <class Team>
PG_HD void run_pass(Graph& g, double* rec, const Team& tm) {
    const int n = 6 * g.F;
    // the live edges, compacted: every loop and every sum over edges runs over this list, so that a graph with edges masked out
    // computes bit for bit what the same graph without those edges computes
    if (tm.tid == 0) {
        int c = 0;
        for (int e = 0; e < g.E; ++e)
            if (g.live[e]) g.lidx[c++] = e;
        g.lidx[g.E] = c;
    }
    tm.sync();
    double s = 0.0;
    for (int j = tm.tid; j < g.lidx[g.E]; j += tm.nt) s += g.info[(size_t)g.lidx[j] * 36 + 35];
    s = tm.sum(s);
    const double cnt = (double)g.lidx[g.E];
    const double w = cnt > 0.0 ? (g.preference * (g.max_distance * g.max_distance)) * (s / cnt) : 0.0;
    double ref0[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) ref0[k] = g.poses[(size_t)g.reference * 16 + k];

    long long t_system = 0, t_solve = 0, c0 = tm.clock();
    evaluate_edges(g, g.poses, true, tm);
    double cur = objective(g, w, tm);
    update_confidence(g, w, tm);
    build_system(g, tm);
    t_system += tm.clock() - c0;
    double lam = 1e-5 * max_of(g.H, n, n + 1, tm), nu = 2.0;
    bool stop = max_of(g.b, n, 1, tm) < 1e-6;
    double xnorm = pose_vector_norm(g, g.poses, tm);
    int iter = 0, solves = 0;
    for (; !stop; ++iter) {
        int lm = 0;
        double rho = 0.0;
        do {
            c0 = tm.clock();
            solve_spd(g.H, g.b, lam, n, g.L, g.delta, g.panel, g.dblk, tm);
            t_solve += tm.clock() - c0;
            ++solves;
            double dd = 0.0, db = 0.0;
            for (int i = tm.tid; i < n; i += tm.nt) {
                const double d = g.delta[i];
                dd += d * d;
                db += d * (lam * d + g.b[i]);
            }
            dd = tm.sum(dd);
            db = tm.sum(db);
            stop = stop || sqrt(dd) < 1e-6 * (xnorm + 1e-6);
            if (!stop) {
                for (int i = tm.tid; i < g.F; i += tm.nt) {
                    double d[6], D[16], P[16], O[16];
#pragma unroll
                    for (int k = 0; k < 6; ++k) d[k] = g.delta[6 * i + k];
#pragma unroll
                    for (int k = 0; k < 16; ++k) P[k] = g.poses[(size_t)i * 16 + k];
                    vec2mat(d, D);
                    mul44(D, P, O);
#pragma unroll
                    for (int k = 0; k < 16; ++k) g.trial[(size_t)i * 16 + k] = O[k];
                }
                tm.sync();
                evaluate_edges(g, g.trial, false, tm);
                const double fresh = objective(g, w, tm);
                rho = (cur - fresh) / (db + 1e-3);
                if (rho > 0.0) {
                    stop = stop || (cur - fresh) < 1e-6 * cur;
                    if (stop) break;
                    const double a = 2.0 * rho - 1.0;
                    lam *= fmax(1.0 / 3.0, fmin(1.0 - (a * a) * a, 2.0 / 3.0));
                    nu = 2.0;
                    cur = fresh;
                    double* t = g.poses; g.poses = g.trial; g.trial = t;
                    xnorm = pose_vector_norm(g, g.poses, tm);
                    c0 = tm.clock();
                    evaluate_edges(g, g.poses, true, tm);
                    update_confidence(g, w, tm);
                    build_system(g, tm);
                    t_system += tm.clock() - c0;
                    stop = stop || max_of(g.b, n, 1, tm) < 1e-6;
                    if (stop) break;
                } else {
                    lam *= nu;
                    nu *= 2.0;
                }
            }
            ++lm;
            stop = stop || lm >= 20;
        } while (!(rho > 0.0 || stop));
        stop = stop || iter >= 100 || cur < 1e-6;
    }
    // open3d does not fix the reference node in the solve; it compensates afterwards: pose_i := ref(original) ref(now)^-1 pose_i
    tm.sync();
    {
        double refn[16], refi[16], Cm[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) refn[k] = g.poses[(size_t)g.reference * 16 + k];
        inv_rigid(refn, refi);
        mul44(ref0, refi, Cm);
        for (int i = tm.tid; i < g.F; i += tm.nt) {
            double P[16], O[16];
#pragma unroll
            for (int k = 0; k < 16; ++k) P[k] = g.poses[(size_t)i * 16 + k];
            mul44(Cm, P, O);
#pragma unroll
            for (int k = 0; k < 16; ++k) g.trial[(size_t)i * 16 + k] = O[k];
        }
        tm.sync();
        double* t = g.poses; g.poses = g.trial; g.trial = t;
    }
    if (tm.tid == 0) {
        rec[0] = (double)iter; rec[1] = (double)solves; rec[2] = cur; rec[3] = w;
        if (g.ticks) { g.ticks[0] += t_system; g.ticks[1] += t_solve; }
    }
}

// global_optimization of one graph: validity, incidence lists, pass 1, prune, pass 2, prune.
// rec: [0] status, [1..4] pass 1 (outer iterations, solves, final objective, w), [5..8] pass 2, [9..11] live edges at the start /
// after the first pruning / at the end.
template <class Team>
PG_HD void run_graph(Graph g, const Team& tm) {
    const int F = g.F, E = g.E;
    const long long begin = tm.clock();
    if (g.ticks && tm.tid == 0) g.ticks[0] = g.ticks[1] = g.ticks[2] = 0;
    bool bad = g.reference < 0 || g.reference >= F;
    double nlive = 0.0;
    for (int e = tm.tid; e < E; e += tm.nt) {
        const bool lv = g.live_in ? g.live_in[e] != 0 : true;
        g.live[e] = lv ? 1 : 0;
        g.conf[e] = 1.0;
        if (!lv) continue;
        nlive += 1.0;
        const int s = g.src[e], t = g.tgt[e];
        bad = bad || s < 0 || s >= F || t < 0 || t >= F || s == t;
        for (int k = 0; k < 16; ++k) bad = bad || !finite_d(g.X[(size_t)e * 16 + k]);
        for (int k = 0; k < 36; ++k) bad = bad || !finite_d(g.info[(size_t)e * 36 + k]);
    }
    for (int i = tm.tid; i < 16 * F; i += tm.nt) bad = bad || !finite_d(g.nodes_in[i]);
    bad = tm.any(bad);
    nlive = tm.sum(nlive);
    for (int k = tm.tid; k < REC; k += tm.nt) g.rec[k] = k == 0 ? (bad ? 1.0 : 0.0) : (k >= 9 ? nlive : 0.0);
    if (bad || nlive == 0.0) {
        for (int i = tm.tid; i < 16 * F; i += tm.nt) g.nodes_out[i] = bad ? (double)NAN : g.nodes_in[i];
        return;
    }
    for (int i = tm.tid; i < 16 * F; i += tm.nt) g.poses[i] = g.nodes_in[i];
    // incidence lists by counting: the edges of node i in ascending index (edges that are not live now never will be)
    for (int i = tm.tid; i < F; i += tm.nt) {
        int c = 0;
        for (int e = 0; e < E; ++e) c += g.live[e] && (g.src[e] == i || g.tgt[e] == i) ? 1 : 0;
        g.inc_start[i + 1] = c;
    }
    tm.sync();
    if (tm.tid == 0) {
        g.inc_start[0] = 0;
        for (int i = 0; i < F; ++i) g.inc_start[i + 1] += g.inc_start[i];
    }
    tm.sync();
    for (int i = tm.tid; i < F; i += tm.nt) {
        int c = g.inc_start[i];
        for (int e = 0; e < E; ++e)
            if (g.live[e] && (g.src[e] == i || g.tgt[e] == i)) g.inc[c++] = e;
    }
    tm.sync();
    for (int pass = 0; pass < 2; ++pass) {
        run_pass(g, g.rec + 1 + 4 * pass, tm);
        double left = 0.0;
        for (int e = tm.tid; e < E; e += tm.nt) {
            if (!g.live[e]) continue;
            if (g.uncertain[e] && !(g.conf[e] > g.prune_threshold)) g.live[e] = 0;
            else left += 1.0;
        }
        left = tm.sum(left);
        if (tm.tid == 0) g.rec[10 + pass] = left;
        tm.sync();
    }
    for (int i = tm.tid; i < 16 * F; i += tm.nt) g.nodes_out[i] = g.poses[i];
    if (g.ticks && tm.tid == 0) g.ticks[2] = tm.clock() - begin;
}

// the driver's node chain (multiway/test_multi_ate.py:129-130): node 0 = I; per live certain edge in order odometry := X odometry,
// next node := odometry^-1 (INVERSE_RULE).  Nodes the chain does not reach are NaN.  One thread.
PG_HD void node_chain(const double* X, const unsigned char* uncertain, const unsigned char* live, int E, int F, double* nodes) {
    double odo[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) odo[k] = (k % 5) == 0 ? 1.0 : 0.0;
    int count = 0;
    if (F > 0) {
#pragma unroll
        for (int k = 0; k < 16; ++k) nodes[k] = odo[k];
        count = 1;
    }
    for (int e = 0; e < E && count < F; ++e) {
        if (uncertain[e] || (live && !live[e])) continue;
        double x[16], nx[16], inv[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) x[k] = X[(size_t)e * 16 + k];
        mul44(x, odo, nx);
        inv_rigid(nx, inv);
#pragma unroll
        for (int k = 0; k < 16; ++k) { odo[k] = nx[k]; nodes[(size_t)count * 16 + k] = inv[k]; }
        ++count;
    }
    for (int i = count * 16; i < F * 16; ++i) nodes[i] = (double)NAN;
}

}  // namespace pg
}  // namespace pdsc
