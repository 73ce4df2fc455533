// f-5: the evaluation's optional ICP post-step (evaluation/test_3DMatch.py:79-80, test_KITTI.py:79-80, multiway/test_multi.py:53-54
// -> evaluation/benchmark_utils.py:40-56 icp_refine): open3d 0.9 registration_icp, point-to-point, on the device.
//   reference algorithm (open3d 0.9 RegistrationICP / GetRegistrationResultAndCorrespondences / TransformationEstimationPointToPoint,
//   restated in DESIGN.md section 8 f-5): fp64 throughout; P = S transformed by init; evaluate; up to max_iteration times
//   {Umeyama of the correspondences, T = U T, P = U P, evaluate, stop when fitness and rmse both moved less than the criteria}.
// One persistent 512-thread workgroup per pair runs the whole loop.  The target never moves: the workgroup first counting-sorts it
// into a hashed 3-D cell grid (cells of width >= r (1 + 1e-3)), then every evaluation looks up the 27 neighbouring cells of each
// transformed source point.  Per iteration: two passes over the source (transform + search + fp64 first-moment sums; demeaned
// covariance), one fp64 Jacobi SVD in thread 0.  Bound: latency (one workgroup per pair); reported as time only.
#include "icp_grid.h"

namespace pdsc {
namespace {

struct IcpLayout {
    size_t tgt, P, corr, cells, cursor, pair_bytes;
    int hmax;
};

inline IcpLayout icp_layout(int Ns, int Nt) {
    IcpLayout L;
    L.hmax = icp_hash_size(Nt);
    size_t o = 0;
    L.tgt = o;    o += (size_t)round_up((long long)Nt * 16, 256);          // sorted target: float4 {x, y, z, original index}
    L.P = o;      o += (size_t)round_up((long long)Ns * 24, 256);          // transformed source, fp64
    L.corr = o;   o += (size_t)round_up((long long)Ns * 4, 256);           // sorted position of each source point's target, -1 = none
    L.cells = o;  o += (size_t)round_up((long long)(L.hmax + 1) * 4, 256); // bucket counts, then bucket starts
    L.cursor = o; o += (size_t)round_up((long long)L.hmax * 4, 256);       // scatter cursors
    L.pair_bytes = o;
    return L;
}

__global__ __launch_bounds__(ICP_NT) void icp_kernel(const float* __restrict__ src, const float* __restrict__ tgt,
                                                     const float* __restrict__ init, const int* __restrict__ ns_per_pair,
                                                     const int* __restrict__ nt_per_pair, double rdist, double r2,
                                                     double rel_fitness, double rel_rmse, int max_iteration,
                                                     float* __restrict__ out_f32, double* __restrict__ out_f64,
                                                     double* __restrict__ fitness_out, double* __restrict__ rmse_out,
                                                     int* __restrict__ ncorr_out, int* __restrict__ iters_out,
                                                     unsigned char* __restrict__ workspace, IcpLayout L, int Ns, int Nt) {
    __shared__ double Tc[16];          // accumulated pose
    __shared__ double Uc[16];          // this iteration's update (the first pass: init)
    __shared__ double red[ICP_NW * 9];
    __shared__ float bb[ICP_NW * 6];
    __shared__ int scan[ICP_NT];
    __shared__ IcpGrid grid_s;
    __shared__ int skip_init;

    const int b = blockIdx.x, t = threadIdx.x;
    int ns = ns_per_pair ? ns_per_pair[b] : Ns;
    int nt = nt_per_pair ? nt_per_pair[b] : Nt;
    ns = ns < 0 ? 0 : (ns > Ns ? Ns : ns);
    nt = nt < 0 ? 0 : (nt > Nt ? Nt : nt);
    const float* srcb = src + (size_t)b * Ns * 3;
    const float* tgtb = tgt + (size_t)b * Nt * 3;
    unsigned char* wb = workspace + (size_t)b * L.pair_bytes;
    float4* tsort = reinterpret_cast<float4*>(wb + L.tgt);
    double* P = reinterpret_cast<double*>(wb + L.P);
    int* corr = reinterpret_cast<int*>(wb + L.corr);
    int* cells = reinterpret_cast<int*>(wb + L.cells);
    int* cursor = reinterpret_cast<int*>(wb + L.cursor);

    if (t < 16) Tc[t] = (double)init[(size_t)b * 16 + t];
    __syncthreads();

    auto finish = [&](double fit, double rmse, int nc, int iters, bool nan_pose) {
        if (t < 16) {
            const double v = nan_pose ? __builtin_nan("") : Tc[t];
            out_f32[(size_t)b * 16 + t] = (float)v;
            if (out_f64) out_f64[(size_t)b * 16 + t] = v;
        }
        if (t == 0) {
            fitness_out[b] = fit;
            rmse_out[b] = rmse;
            ncorr_out[b] = nc;
            iters_out[b] = iters;
        }
    };

    // open3d: max_correspondence_distance <= 0 returns RegistrationResult(init) before looking at any point
    if (!(rdist > 0.0)) { finish(0.0, 0.0, 0, 0, false); return; }

    // ---- finiteness of init and of every valid point; target bounding box (fp32 min / max: exact) ----
    bool bad = t < 16 && !isfinite(Tc[t]);
    for (int i = t; i < ns; i += ICP_NT) bad |= !finite3(srcb[i * 3], srcb[i * 3 + 1], srcb[i * 3 + 2]);
    float mn[3], mx[3];
    bad |= cloud_bounds(tgtb, nt, mn, mx);
    // a non-finite init or point: NaN pose, never a plausible one (a NaN pose of the forward's range sentinel stays NaN)
    if (__syncthreads_or(bad)) { finish(__builtin_nan(""), __builtin_nan(""), 0, 0, true); return; }
    icp_make_grid(mn, mx, nt, rdist, bb, &grid_s);
    // Eigen isIdentity(): skip the init transform of the source when it passes
    if (t == 0) skip_init = icp_is_identity(Tc) ? 1 : 0;
    __syncthreads();
    const IcpGrid g = grid_s;

    // ---- counting sort of the target into the grid's buckets ----
    icp_sort_target(tgtb, nt, g, cells, cursor, tsort, scan);
    if (t < 16) Uc[t] = Tc[t];
    __syncthreads();

    // ---- evaluate(P) after P = U P (the first pass: P = init S, or S when init passes isIdentity) ----
    // acc: |corr|, sum d2, sum p (3), sum q (3)
    auto evaluate = [&](bool first, double (&acc)[9]) {
#pragma unroll
        for (int k = 0; k < 9; ++k) acc[k] = 0.0;
        const bool apply = !(first && skip_init);
        for (int i = t; i < ns; i += ICP_NT) {
            double x, y, z;
            if (first) { x = srcb[i * 3]; y = srcb[i * 3 + 1]; z = srcb[i * 3 + 2]; }
            else { x = P[i * 3]; y = P[i * 3 + 1]; z = P[i * 3 + 2]; }
            if (apply) {
                // Eigen: (U * (x, y, z, 1)).head<3>() / w; w == 1 for every update and for a rigid init
                const double nx = Uc[0] * x + Uc[1] * y + Uc[2] * z + Uc[3];
                const double ny = Uc[4] * x + Uc[5] * y + Uc[6] * z + Uc[7];
                const double nz = Uc[8] * x + Uc[9] * y + Uc[10] * z + Uc[11];
                const double w = Uc[12] * x + Uc[13] * y + Uc[14] * z + Uc[15];
                x = nx / w; y = ny / w; z = nz / w;
            }
            P[i * 3] = x; P[i * 3 + 1] = y; P[i * 3 + 2] = z;
            double d2;
            const int j = icp_nearest(x, y, z, g, tsort, cells, r2, d2);
            corr[i] = j;
            if (j >= 0) {
                const float4 q = tsort[j];
                acc[0] += 1.0; acc[1] += d2;
                acc[2] += x; acc[3] += y; acc[4] += z;
                acc[5] += (double)q.x; acc[6] += (double)q.y; acc[7] += (double)q.z;
            }
        }
        block_sum_f64<9>(acc, red);
    };

    double acc[9];
    evaluate(true, acc);
    int n = (int)acc[0];
    double fit = n > 0 ? (double)n / (double)ns : 0.0;
    double rmse = n > 0 ? sqrt(acc[1] / (double)n) : 0.0;
    int it = 0;
    while (it < max_iteration) {
        // ---- U = umeyama(P[corr], Q[corr]) (Eigen::umeyama, no scaling); identity for an empty set ----
        __syncthreads();                               // everyone is done reading Uc
        if (n > 0) {
            const double one_over_n = 1.0 / (double)n;
            const double mA[3] = {acc[2] * one_over_n, acc[3] * one_over_n, acc[4] * one_over_n};
            const double mB[3] = {acc[5] * one_over_n, acc[6] * one_over_n, acc[7] * one_over_n};
            double H[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
            for (int i = t; i < ns; i += ICP_NT) {
                const int j = corr[i];
                if (j < 0) continue;
                const float4 q = tsort[j];
                const double a[3] = {P[i * 3] - mA[0], P[i * 3 + 1] - mA[1], P[i * 3 + 2] - mA[2]};
                const double bq[3] = {(double)q.x - mB[0], (double)q.y - mB[1], (double)q.z - mB[2]};
#pragma unroll
                for (int r = 0; r < 3; ++r)
#pragma unroll
                    for (int c = 0; c < 3; ++c) H[r * 3 + c] += a[r] * bq[c];
            }
            block_sum_f64<9>(H, red);
            if (t == 0) {
#pragma unroll
                for (int k = 0; k < 9; ++k) H[k] *= one_over_n;
                double U[16];
                kabsch_from_covariance_f64(H, mA, mB, U);
                double Tn[16];
                for (int r = 0; r < 4; ++r)
                    for (int c = 0; c < 4; ++c)
                        Tn[r * 4 + c] = U[r * 4 + 0] * Tc[0 * 4 + c] + U[r * 4 + 1] * Tc[1 * 4 + c] + U[r * 4 + 2] * Tc[2 * 4 + c] +
                                        U[r * 4 + 3] * Tc[3 * 4 + c];
                for (int k = 0; k < 16; ++k) { Uc[k] = U[k]; Tc[k] = Tn[k]; }
            }
        } else if (t < 16) {
            Uc[t] = (t % 5) == 0 ? 1.0 : 0.0;
        }
        __syncthreads();
        const double prev_fit = fit, prev_rmse = rmse;
        evaluate(false, acc);
        ++it;
        n = (int)acc[0];
        fit = n > 0 ? (double)n / (double)ns : 0.0;
        rmse = n > 0 ? sqrt(acc[1] / (double)n) : 0.0;
        if (fabs(prev_fit - fit) < rel_fitness && fabs(prev_rmse - rmse) < rel_rmse) break;
    }
    __syncthreads();
    finish(fit, rmse, n, it, false);
}

}  // namespace

size_t icp_workspace_bytes(int bs, int Ns, int Nt) {
    if (bs <= 0 || Ns <= 0 || Nt <= 0) return 0;
    return icp_layout(Ns, Nt).pair_bytes * (size_t)bs;
}

int launch_icp_refine(const float* src, const float* tgt, const float* init, const int* ns_per_pair, const int* nt_per_pair,
                      double max_distance, double relative_fitness, double relative_rmse, int max_iteration, float* out_f32,
                      double* out_f64, double* fitness, double* inlier_rmse, int* num_corr, int* iterations, void* workspace,
                      size_t workspace_bytes, int bs, int Ns, int Nt, hipStream_t st) {
    PDSC_REQUIRE(src && tgt && init && out_f32 && fitness && inlier_rmse && num_corr && iterations && workspace,
                 "pdsc_icp_refine: null pointer");
    PDSC_REQUIRE(bs > 0 && Ns > 0 && Nt > 0 && max_iteration >= 0, "pdsc_icp_refine: bs=%d Ns=%d Nt=%d max_iteration=%d", bs, Ns, Nt,
                 max_iteration);
    PDSC_REQUIRE(Ns <= (1 << 24) && Nt <= (1 << 24), "pdsc_icp_refine: Ns=%d Nt=%d above 2^24", Ns, Nt);
    PDSC_REQUIRE(!isnan(max_distance) && !isnan(relative_fitness) && !isnan(relative_rmse),
                 "pdsc_icp_refine: NaN max_distance / criteria");
    const IcpLayout L = icp_layout(Ns, Nt);
    PDSC_REQUIRE(workspace_bytes >= L.pair_bytes * (size_t)bs, "pdsc_icp_refine: workspace %zu bytes < %zu", workspace_bytes,
                 L.pair_bytes * (size_t)bs);
    // FLANN's radius search takes the squared radius as float: float(r * r), compared with '<' against the fp64 distance
    const double r2 = max_distance > 0.0 ? (double)(float)(max_distance * max_distance) : 0.0;
    hipLaunchKernelGGL(icp_kernel, dim3(bs), dim3(ICP_NT), 0, st, src, tgt, init, ns_per_pair, nt_per_pair, max_distance, r2,
                       relative_fitness, relative_rmse, max_iteration, out_f32, out_f64, fitness, inlier_rmse, num_corr, iterations,
                       (unsigned char*)workspace, L, Ns, Nt);
    return check_launch("pdsc_icp_refine");
}

}  // namespace pdsc

extern "C" size_t pdsc_icp_workspace_bytes(int bs, int Ns, int Nt) { return pdsc::icp_workspace_bytes(bs, Ns, Nt); }

extern "C" int pdsc_icp_refine(const float* src, const float* tgt, const float* init_trans, const int* Ns_per_pair,
                               const int* Nt_per_pair, double max_distance, double relative_fitness, double relative_rmse,
                               int max_iteration, float* out_trans_f32, double* out_trans_f64, double* fitness, double* inlier_rmse,
                               int* num_corr, int* iterations, void* workspace, size_t workspace_bytes, int bs, int Ns, int Nt,
                               void* stream) {
    return pdsc::launch_icp_refine(src, tgt, init_trans, Ns_per_pair, Nt_per_pair, max_distance, relative_fitness, relative_rmse,
                                   max_iteration, out_trans_f32, out_trans_f64, fitness, inlier_rmse, num_corr, iterations, workspace,
                                   workspace_bytes, bs, Ns, Nt, (hipStream_t)stream);
}
