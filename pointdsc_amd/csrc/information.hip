// f-6: the multiway driver's edge information (multiway/test_multi_ate.py:69-72, :141-146): open3d
// registration.get_information_matrix_from_point_clouds (GetInformationMatrixFromPointClouds) on the device.
//   reference algorithm (restated in DESIGN.md section 8 f-6): fp64 throughout; P = T S (skipped when T passes Eigen's
//   isIdentity(), as in the ICP); the correspondence set is the ICP's evaluate step (nearest target with d2 < float(r r), lowest
//   target index among equal distances: FLANN_RADIUS_RULE / TIE_RULE of f-5); for every correspondence with TARGET point (x, y, z)
//   GTG += g g^T for the three rows g = (0, z, -y, 1, 0, 0), (-z, 0, x, 0, 1, 0), (y, -x, 0, 0, 0, 1).
//   IDENTITY_RULE: open3d 0.9 is believed to start each OpenMP thread's private accumulator from the 6x6 identity, so that its
//   result carries + (threads used) on the diagonal; later versions start from zero.  That cannot be checked without open3d; this
//   kernel returns the plain sum (the later versions' result), so [3][3] = [4][4] = [5][5] = |corr| exactly.
// One 512-thread workgroup per pair: counting sort of the target into the cell grid of icp_grid.h, one pass over the source
// (transform + search + sums).  The matrix has 9 sums that differ in more than sign -- x, y, z, xy, xz, yz, y^2 + z^2, x^2 + z^2,
// x^2 + y^2 (the squares added one after the other, as the three rank-one updates do) -- plus the count; -x, -y, -z are the exact
// negations of the sums (rounding is symmetric; written 0 - s so that an empty set gives +0).  fp64 in a fixed order
// (block_sum_f64).  Bound: latency, as the ICP.
#include "icp_grid.h"

namespace pdsc {
namespace {

struct InfoLayout {
    size_t tgt, cells, cursor, pair_bytes;
};

inline InfoLayout info_layout(int Nt) {
    InfoLayout L;
    const int hmax = icp_hash_size(Nt);
    size_t o = 0;
    L.tgt = o;    o += (size_t)round_up((long long)Nt * 16, 256);          // sorted target: float4 {x, y, z, original index}
    L.cells = o;  o += (size_t)round_up((long long)(hmax + 1) * 4, 256);   // bucket counts, then bucket starts
    L.cursor = o; o += (size_t)round_up((long long)hmax * 4, 256);         // scatter cursors
    L.pair_bytes = o;
    return L;
}

constexpr int INFO_NV = 10;   // |corr|, sum x, y, z, xy, xz, yz, y2 + z2, x2 + z2, x2 + y2

__global__ __launch_bounds__(ICP_NT) void information_kernel(const float* __restrict__ src, const float* __restrict__ tgt,
                                                             const float* __restrict__ trans, const int* __restrict__ ns_per_pair,
                                                             const int* __restrict__ nt_per_pair, double rdist, double r2,
                                                             double* __restrict__ info, int* __restrict__ ncorr_out,
                                                             int* __restrict__ corr_out, unsigned char* __restrict__ workspace,
                                                             InfoLayout L, int Ns, int Nt) {
    __shared__ double Tc[16];
    __shared__ double red[ICP_NW * INFO_NV];
    __shared__ float bb[ICP_NW * 6];
    __shared__ int scan[ICP_NT];
    __shared__ IcpGrid grid_s;
    __shared__ int skip_s;

    const int b = blockIdx.x, t = threadIdx.x;
    int ns = ns_per_pair ? ns_per_pair[b] : Ns;
    int nt = nt_per_pair ? nt_per_pair[b] : Nt;
    ns = ns < 0 ? 0 : (ns > Ns ? Ns : ns);
    nt = nt < 0 ? 0 : (nt > Nt ? Nt : nt);
    const float* srcb = src + (size_t)b * Ns * 3;
    const float* tgtb = tgt + (size_t)b * Nt * 3;
    unsigned char* wb = workspace + (size_t)b * L.pair_bytes;
    float4* tsort = reinterpret_cast<float4*>(wb + L.tgt);
    int* cells = reinterpret_cast<int*>(wb + L.cells);
    int* cursor = reinterpret_cast<int*>(wb + L.cursor);
    double* infob = info + (size_t)b * 36;
    int* corrb = corr_out ? corr_out + (size_t)b * Ns : nullptr;

    if (t < 16) Tc[t] = (double)trans[(size_t)b * 16 + t];
    __syncthreads();

    // the same value in all 36 entries, no correspondence
    auto constant_result = [&](double v) {
        if (t < 36) infob[t] = v;
        if (t == 0) ncorr_out[b] = 0;
        if (corrb)
            for (int i = t; i < Ns; i += ICP_NT) corrb[i] = -1;
    };

    // max_correspondence_distance <= 0: no point can be within it
    if (!(rdist > 0.0)) { constant_result(0.0); return; }

    bool bad = t < 16 && !isfinite(Tc[t]);
    for (int i = t; i < ns; i += ICP_NT) bad |= !finite3(srcb[i * 3], srcb[i * 3 + 1], srcb[i * 3 + 2]);
    float mn[3], mx[3];
    bad |= cloud_bounds(tgtb, nt, mn, mx);
    // a non-finite pose or point: a NaN matrix, never a plausible one
    if (__syncthreads_or(bad)) { constant_result(__builtin_nan("")); return; }
    icp_make_grid(mn, mx, nt, rdist, bb, &grid_s);
    if (t == 0) skip_s = icp_is_identity(Tc) ? 1 : 0;
    __syncthreads();
    const IcpGrid g = grid_s;
    icp_sort_target(tgtb, nt, g, cells, cursor, tsort, scan);
    __syncthreads();

    const bool apply = !skip_s;
    double acc[INFO_NV];
#pragma unroll
    for (int k = 0; k < INFO_NV; ++k) acc[k] = 0.0;
    for (int i = t; i < ns; i += ICP_NT) {
        double px = srcb[i * 3], py = srcb[i * 3 + 1], pz = srcb[i * 3 + 2];
        if (apply) {
            // Eigen: (T * (x, y, z, 1)).head<3>() / w, in the ICP kernel's order
            const double nx = Tc[0] * px + Tc[1] * py + Tc[2] * pz + Tc[3];
            const double ny = Tc[4] * px + Tc[5] * py + Tc[6] * pz + Tc[7];
            const double nz = Tc[8] * px + Tc[9] * py + Tc[10] * pz + Tc[11];
            const double w = Tc[12] * px + Tc[13] * py + Tc[14] * pz + Tc[15];
            px = nx / w; py = ny / w; pz = nz / w;
        }
        double d2;
        const int j = icp_nearest(px, py, pz, g, tsort, cells, r2, d2);
        int orig = -1;
        if (j >= 0) {
            const float4 q = tsort[j];
            orig = __float_as_int(q.w);
            const double x = q.x, y = q.y, z = q.z;
            acc[0] += 1.0;
            acc[1] += x; acc[2] += y; acc[3] += z;
            acc[4] += x * y; acc[5] += x * z; acc[6] += y * z;
            // [0][0]: rows (0, z, -y, ..) then (-z, 0, x, ..) then (y, -x, 0, ..) add 0, z z, y y in this order; likewise [1][1], [2][2]
            acc[7] += z * z; acc[7] += y * y;
            acc[8] += z * z; acc[8] += x * x;
            acc[9] += y * y; acc[9] += x * x;
        }
        if (corrb) corrb[i] = orig;
    }
    if (corrb)
        for (int i = ns + t; i < Ns; i += ICP_NT) corrb[i] = -1;
    block_sum_f64<INFO_NV>(acc, red);
    if (t < 36) {
        const int r = t / 6, c = t % 6;
        const int lo = r < c ? r : c, hi = r < c ? c : r;
        const double n = acc[0], sx = acc[1], sy = acc[2], sz = acc[3];
        double v = 0.0;
        if (lo == hi) v = lo == 0 ? acc[7] : (lo == 1 ? acc[8] : (lo == 2 ? acc[9] : n));
        else if (lo == 0 && hi == 1) v = 0.0 - acc[4];
        else if (lo == 0 && hi == 2) v = 0.0 - acc[5];
        else if (lo == 1 && hi == 2) v = 0.0 - acc[6];
        else if (lo == 0 && hi == 4) v = 0.0 - sz;
        else if (lo == 0 && hi == 5) v = sy;
        else if (lo == 1 && hi == 3) v = sz;
        else if (lo == 1 && hi == 5) v = 0.0 - sx;
        else if (lo == 2 && hi == 3) v = 0.0 - sy;
        else if (lo == 2 && hi == 4) v = sx;
        infob[t] = v;
    }
    if (t == 0) ncorr_out[b] = (int)acc[0];
}

}  // namespace

size_t information_workspace_bytes(int bs, int Ns, int Nt) {
    if (bs <= 0 || Ns <= 0 || Nt <= 0) return 0;
    return info_layout(Nt).pair_bytes * (size_t)bs;
}

int launch_information_matrix(const float* src, const float* tgt, const float* trans, const int* ns_per_pair, const int* nt_per_pair,
                              double max_distance, double* info, int* num_corr, int* corr, void* workspace, size_t workspace_bytes,
                              int bs, int Ns, int Nt, hipStream_t st) {
    PDSC_REQUIRE(src && tgt && trans && info && num_corr && workspace, "pdsc_information_matrix: null pointer");
    PDSC_REQUIRE(bs > 0 && Ns > 0 && Nt > 0, "pdsc_information_matrix: bs=%d Ns=%d Nt=%d", bs, Ns, Nt);
    PDSC_REQUIRE(Ns <= (1 << 24) && Nt <= (1 << 24), "pdsc_information_matrix: Ns=%d Nt=%d above 2^24", Ns, Nt);
    PDSC_REQUIRE(!isnan(max_distance), "pdsc_information_matrix: NaN max_distance");
    const InfoLayout L = info_layout(Nt);
    PDSC_REQUIRE(workspace_bytes >= L.pair_bytes * (size_t)bs, "pdsc_information_matrix: workspace %zu bytes < %zu", workspace_bytes,
                 L.pair_bytes * (size_t)bs);
    // FLANN_RADIUS_RULE of f-5: the squared radius as float(r * r), compared with '<' against the fp64 distance
    const double r2 = max_distance > 0.0 ? (double)(float)(max_distance * max_distance) : 0.0;
    hipLaunchKernelGGL(information_kernel, dim3(bs), dim3(ICP_NT), 0, st, src, tgt, trans, ns_per_pair, nt_per_pair, max_distance, r2,
                       info, num_corr, corr, (unsigned char*)workspace, L, Ns, Nt);
    return check_launch("pdsc_information_matrix");
}

}  // namespace pdsc

extern "C" size_t pdsc_information_workspace_bytes(int bs, int Ns, int Nt) { return pdsc::information_workspace_bytes(bs, Ns, Nt); }

extern "C" int pdsc_information_matrix(const float* src, const float* tgt, const float* trans, const int* Ns_per_pair,
                                       const int* Nt_per_pair, double max_distance, double* info, int* num_corr, int* corr,
                                       void* workspace, size_t workspace_bytes, int bs, int Ns, int Nt, void* stream) {
    return pdsc::launch_information_matrix(src, tgt, trans, Ns_per_pair, Nt_per_pair, max_distance, info, num_corr, corr, workspace,
                                           workspace_bytes, bs, Ns, Nt, (hipStream_t)stream);
}
