// f-7: FPFH descriptors of a down-sampled cloud (misc/cal_fpfh.py:21-26: open3d estimate_normals + compute_fpfh_feature with
// KDTreeSearchParamHybrid, then demo_registration.py:43's f / (|f| + 1e-6)), on the device, fp64 throughout.  The algorithm and
// the three named rules (FLANN_RADIUS_RULE, COVARIANCE_ORDER_RULE, NORMAL_SIGN_RULE) are written out in DESIGN.md section 8 f-7
// and in include/pointdsc_hip.h.  Kernels:
//   nb_grid_kernel    one 512-thread workgroup per cloud counting-sorts the cloud into the hashed cell grid of icp_grid.h
//                     (cells of width r (1 + 1e-3): the 27-cell lookup equals brute force exactly, margin argument there);
//                     f-9, for raw clouds (path many of cloud_many.h): the same grid and the same buckets from a chain of
//                     many-workgroup kernels, cloud_box_kernel (chunk boxes; clears the bucket counts) -> nb_header_kernel (box,
//                     grid) -> nb_hist_kernel -> nb_scan_kernel -> nb_scatter_kernel; only the order inside a bucket differs,
//                     which nb_search_kernel does not see (it ranks by (d2, index));
//   nb_search_kernel  one wavefront per query: lanes over the candidates of the 27 buckets, accepted candidates are appended to an
//                     LDS buffer, and whenever it fills (and once at the end) a rank count by (d2, index) keeps the max_nn
//                     smallest in order; the max_nn-th key then tightens the acceptance test (the cut is the common case:
//                     63-71 % of the demo clouds' points reach max_nn = 100 at r = 0.25);
//   normals_kernel    one wavefront per point: the list is ranked by index (COVARIANCE_ORDER_RULE), nine lanes sum one cumulant
//                     each in that order, lane 0 solves the symmetric 3x3 eigenproblem (cyclic Jacobi, in registers);
//   spfh_kernel       one wavefront per point, lanes over neighbours, a 33-bin count in LDS, scaled by 100 / (count - 1);
//   fpfh_kernel       one wavefront per point, one lane per bin, serial over the neighbours (the oracle's order), the three block
//                     sums accumulated neighbour-major, bin-minor as ComputeFPFHFeature does; L2 normalisation for the fp32 copy.
// The build compiles with -ffp-contract=off, so every expression below is evaluated as written: the squared distances and the
// covariance are bit-equal to an fp64 restatement with the same operation order.  Bound: latency / LDS (small per-point problems);
// reported as time only.
#include "cloud_many.h"

namespace pdsc {
namespace {

constexpr int FPFH_WAVE = 64;
constexpr int FPFH_CAP = 256;                        // candidate buffer of a query (LDS): a selection runs when more than CAP - 64 wait
constexpr int FPFH_MAX_NN = PDSC_FPFH_MAX_NN;
constexpr int FPFH_DIM = PDSC_FPFH_DIM;
static_assert(FPFH_MAX_NN <= FPFH_CAP - FPFH_WAVE, "a selection must leave room for one more round of candidates");

struct NbHeader {
    IcpGrid g;
    int bad;                                         // the cloud holds a non-finite point
};

struct NbLayout {
    size_t tsort, cells, cursor, header, parts, cloud_bytes;
};

inline NbLayout nb_layout(int N) {
    NbLayout L;
    const int hmax = icp_hash_size(N);
    size_t o = 0;
    L.tsort = o;  o += (size_t)round_up((long long)N * 16, 256);             // sorted cloud: float4 {x, y, z, original index}
    L.cells = o;  o += (size_t)round_up((long long)(hmax + 1) * 4, 256);     // bucket counts, then bucket starts
    L.cursor = o; o += (size_t)round_up((long long)hmax * 4, 256);           // scatter cursors
    L.header = o; o += (size_t)round_up((long long)sizeof(NbHeader), 256);
    L.parts = o;  o += (size_t)round_up((long long)cloud_chunks(N) * (long long)sizeof(CloudBox), 256);   // chunk boxes (path many)
    L.cloud_bytes = o;
    return L;
}

// ---- a. neighbour lists ----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(ICP_NT) void nb_grid_kernel(const float* __restrict__ points, const int* __restrict__ n_per_cloud,
                                                         double rdist, unsigned char* __restrict__ workspace, NbLayout L, int N) {
    __shared__ float bb[ICP_NW * 6];
    __shared__ int scan[ICP_NT];
    __shared__ IcpGrid grid_s;
    const int b = blockIdx.x, t = threadIdx.x;
    const int n = cloud_count(n_per_cloud, b, N);
    const float* pb = points + (size_t)b * N * 3;
    unsigned char* wb = workspace + (size_t)b * L.cloud_bytes;
    NbHeader* hdr = reinterpret_cast<NbHeader*>(wb + L.header);

    float mn[3], mx[3];
    const bool bad = cloud_bounds(pb, n, mn, mx);
    if (__syncthreads_or(bad)) {
        if (t == 0) hdr->bad = 1;
        return;
    }
    icp_make_grid(mn, mx, n, rdist, bb, &grid_s);
    __syncthreads();
    const IcpGrid g = grid_s;
    icp_sort_target(pb, n, g, reinterpret_cast<int*>(wb + L.cells), reinterpret_cast<int*>(wb + L.cursor),
                    reinterpret_cast<float4*>(wb + L.tsort), scan);
    if (t == 0) {
        hdr->g = g;
        hdr->bad = 0;
    }
}

// ---- a'. the same grid from many workgroups per cloud (f-9) -------------------------------------------------------------------
// one workgroup per cloud: the chunks' boxes -> the header (the grid of icp_make_grid over the same box)
__global__ __launch_bounds__(ICP_NT) void nb_header_kernel(const int* __restrict__ n_per_cloud, double rdist,
                                                           unsigned char* __restrict__ workspace, NbLayout L, int N) {
    __shared__ float bb[ICP_NW * 6];
    __shared__ IcpGrid grid_s;
    const int b = blockIdx.x, t = threadIdx.x;
    const int n = cloud_count(n_per_cloud, b, N);
    unsigned char* wb = workspace + (size_t)b * L.cloud_bytes;
    NbHeader* hdr = reinterpret_cast<NbHeader*>(wb + L.header);
    float mn[3], mx[3];
    const bool bad = cloud_box_share(reinterpret_cast<const CloudBox*>(wb + L.parts), cloud_chunks(N), mn, mx);
    if (__syncthreads_or(bad)) {
        if (t == 0) hdr->bad = 1;
        return;
    }
    icp_make_grid(mn, mx, n, rdist, bb, &grid_s);
    __syncthreads();
    if (t == 0) {
        hdr->g = grid_s;
        hdr->bad = 0;
    }
}

// grid (nchunk, bs): bucket counts (cleared by cloud_box_kernel)
__global__ __launch_bounds__(ICP_NT) void nb_hist_kernel(const float* __restrict__ points, const int* __restrict__ n_per_cloud,
                                                         unsigned char* __restrict__ workspace, NbLayout L, int N) {
    const int c = blockIdx.x, b = blockIdx.y, t = threadIdx.x;
    const int n = cloud_count(n_per_cloud, b, N);
    const float* pb = points + (size_t)b * N * 3;
    unsigned char* wb = workspace + (size_t)b * L.cloud_bytes;
    const NbHeader* hdr = reinterpret_cast<const NbHeader*>(wb + L.header);
    if (hdr->bad) return;
    const IcpGrid g = hdr->g;
    int* cells = reinterpret_cast<int*>(wb + L.cells);
    const int i1 = min((c + 1) * CLOUD_CHUNK, n);
    for (int i = c * CLOUD_CHUNK + t; i < i1; i += ICP_NT) atomicAdd(&cells[icp_target_bucket(pb[i * 3], pb[i * 3 + 1], pb[i * 3 + 2], g)], 1);
}

// one workgroup per cloud: bucket counts -> bucket starts and scatter cursors
__global__ __launch_bounds__(ICP_NT) void nb_scan_kernel(unsigned char* __restrict__ workspace, NbLayout L) {
    __shared__ int scan[ICP_NT];
    unsigned char* wb = workspace + (size_t)blockIdx.x * L.cloud_bytes;
    const NbHeader* hdr = reinterpret_cast<const NbHeader*>(wb + L.header);
    if (hdr->bad) return;
    icp_scan_cells(reinterpret_cast<int*>(wb + L.cells), reinterpret_cast<int*>(wb + L.cursor), hdr->g.hmask + 1, scan);
}

// grid (nchunk, bs)
__global__ __launch_bounds__(ICP_NT) void nb_scatter_kernel(const float* __restrict__ points, const int* __restrict__ n_per_cloud,
                                                            unsigned char* __restrict__ workspace, NbLayout L, int N) {
    const int c = blockIdx.x, b = blockIdx.y, t = threadIdx.x;
    const int n = cloud_count(n_per_cloud, b, N);
    const float* pb = points + (size_t)b * N * 3;
    unsigned char* wb = workspace + (size_t)b * L.cloud_bytes;
    const NbHeader* hdr = reinterpret_cast<const NbHeader*>(wb + L.header);
    if (hdr->bad) return;
    const IcpGrid g = hdr->g;
    int* cursor = reinterpret_cast<int*>(wb + L.cursor);
    float4* tsort = reinterpret_cast<float4*>(wb + L.tsort);
    const int i1 = min((c + 1) * CLOUD_CHUNK, n);
    for (int i = c * CLOUD_CHUNK + t; i < i1; i += ICP_NT) {
        const float x = pb[i * 3], y = pb[i * 3 + 1], z = pb[i * 3 + 2];
        const int pos = atomicAdd(&cursor[icp_target_bucket(x, y, z, g)], 1);
        tsort[pos] = make_float4(x, y, z, __int_as_float(i));          // order inside a bucket is free: the search ranks by (d2, index)
    }
}

__global__ __launch_bounds__(FPFH_WAVE) void nb_search_kernel(const float* __restrict__ points, const int* __restrict__ n_per_cloud,
                                                              double r2, int max_nn, int* __restrict__ idx_out,
                                                              double* __restrict__ d2_out, int* __restrict__ count_out,
                                                              const unsigned char* __restrict__ workspace, NbLayout L, int N) {
    __shared__ double cd2[FPFH_CAP];                 // candidates (the first n_c entries), unordered after the last selection
    __shared__ int cidx[FPFH_CAP];
    __shared__ double sd2[FPFH_MAX_NN];              // the selection's output, ascending by (d2, index)
    __shared__ int sidx[FPFH_MAX_NN];
    const int i = blockIdx.x, b = blockIdx.y, lane = threadIdx.x;
    const int n = cloud_count(n_per_cloud, b, N);
    const size_t row = (size_t)b * N + i;
    int* io = idx_out + row * max_nn;
    double* dout = d2_out ? d2_out + row * max_nn : nullptr;
    const unsigned char* wb = workspace + (size_t)b * L.cloud_bytes;
    const NbHeader* hdr = reinterpret_cast<const NbHeader*>(wb + L.header);

    if (i >= n || hdr->bad) {                        // padding row: an empty list; a cloud with a non-finite point: count -1
        for (int e = lane; e < max_nn; e += FPFH_WAVE) {
            io[e] = -1;
            if (dout) dout[e] = 0.0;
        }
        if (lane == 0) count_out[row] = i >= n ? 0 : -1;
        return;
    }
    const IcpGrid g = hdr->g;
    const float4* tsort = reinterpret_cast<const float4*>(wb + L.tsort);
    const int* cells = reinterpret_cast<const int*>(wb + L.cells);
    const float* pb = points + (size_t)b * N * 3;
    const double px = (double)pb[i * 3], py = (double)pb[i * 3 + 1], pz = (double)pb[i * 3 + 2];

    // the 27 neighbour buckets, one per lane; a bucket that two neighbour cells hash to is scanned once
    int qx = 0, qy = 0, qz = 0;
    const bool any = icp_query_cell(px, g.xmin, g.w, g.nx, qx) && icp_query_cell(py, g.ymin, g.w, g.ny, qy) &&
                     icp_query_cell(pz, g.zmin, g.w, g.nz, qz);
    int h = -1;
    if (lane < 27) {
        const int cx = qx + lane % 3 - 1, cy = qy + (lane / 3) % 3 - 1, cz = qz + lane / 9 - 1;
        if (any && cx >= 0 && cx < g.nx && cy >= 0 && cy < g.ny && cz >= 0 && cz < g.nz) h = icp_bucket(cx, cy, cz, g.hmask);
    }
    bool dup = false;
    for (int k = 0; k < 26; ++k) {
        const int hk = __shfl(h, k, 64);
        dup |= lane > k && hk == h;
    }
    int j0 = 0, j1 = 0;
    if (h >= 0 && !dup) {
        j0 = cells[h];
        j1 = cells[h + 1];
    }

    int n_c = 0;                                     // candidates waiting in cd2 / cidx (the same in every lane)
    double thr_d2 = r2;                              // accepted: (d2, index) < (thr_d2, thr_idx); before the first full selection the
    int thr_idx = -1;                                // radius test d2 < r2 alone
    auto select = [&]() {
        __syncthreads();
        const int keep = n_c < max_nn ? n_c : max_nn;
        for (int e = lane; e < n_c; e += FPFH_WAVE) {
            const double d = cd2[e];
            const int id = cidx[e];
            int rank = 0;
            for (int o = 0; o < n_c; ++o) {
                const double od = cd2[o];
                const int oi = cidx[o];
                rank += (od < d || (od == d && oi < id)) ? 1 : 0;
            }
            if (rank < keep) {                       // indices are distinct, so the ranks are
                sd2[rank] = d;
                sidx[rank] = id;
            }
        }
        __syncthreads();
        for (int e = lane; e < keep; e += FPFH_WAVE) {
            cd2[e] = sd2[e];
            cidx[e] = sidx[e];
        }
        n_c = keep;
        if (keep == max_nn) {
            thr_d2 = sd2[max_nn - 1];
            thr_idx = sidx[max_nn - 1];
        }
        __syncthreads();
    };

    for (int k = 0; k < 27; ++k) {
        const int a0 = __shfl(j0, k, 64), a1 = __shfl(j1, k, 64);
        for (int base = a0; base < a1; base += FPFH_WAVE) {
            const int j = base + lane;
            bool ok = false;
            double d2 = 0.0;
            int id = 0;
            if (j < a1) {
                const float4 q = tsort[j];
                const double dx = px - (double)q.x, dy = py - (double)q.y, dz = pz - (double)q.z;
                d2 = (dx * dx + dy * dy) + dz * dz;
                id = __float_as_int(q.w);
                ok = d2 < thr_d2 || (d2 == thr_d2 && id < thr_idx);
            }
            const unsigned long long m = __ballot(ok);
            if (ok) {
                const int pos = n_c + __popcll(m & ((1ull << lane) - 1ull));      // < n_c + 64 <= FPFH_CAP
                cd2[pos] = d2;
                cidx[pos] = id;
            }
            n_c += __popcll(m);
            if (n_c > FPFH_CAP - FPFH_WAVE) select();
        }
    }
    select();
    for (int e = lane; e < max_nn; e += FPFH_WAVE) {
        io[e] = e < n_c ? sidx[e] : -1;
        if (dout) dout[e] = e < n_c ? sd2[e] : 0.0;
    }
    if (lane == 0) count_out[row] = n_c;
}

// a list entry as a row of its cloud: lists come from the caller in the stage entries, so nothing outside the cloud is ever read
__device__ __forceinline__ int list_row(int id, int n) { return id < 0 ? 0 : (id >= n ? n - 1 : id); }

// ---- b. normals -------------------------------------------------------------------------------------------------------------
// Unit eigenvector of the smallest eigenvalue of the symmetric matrix {c00 c01 c02; c01 c11 c12; c02 c12 c22}: the cyclic Jacobi of
// kabsch3.h, 16 sweeps to 1e-18.
__device__ inline void smallest_eigenvector(double c00, double c01, double c02, double c11, double c12, double c22, double (&nv)[3]) {
    double A[3][3] = {{c00, c01, c02}, {c01, c11, c12}, {c02, c12, c22}};
    double V[3][3];
    jacobi_eig3<16>(A, V, 1e-18);
    const double e0 = A[0][0], e1 = A[1][1], e2 = A[2][2];
    const int m = (e0 <= e1 && e0 <= e2) ? 0 : (e1 <= e2 ? 1 : 2);
    // select the column with compares (runtime-indexed local arrays would go to scratch memory)
    double x = m == 0 ? V[0][0] : (m == 1 ? V[0][1] : V[0][2]);
    double y = m == 0 ? V[1][0] : (m == 1 ? V[1][1] : V[1][2]);
    double z = m == 0 ? V[2][0] : (m == 1 ? V[2][1] : V[2][2]);
    const double len = sqrt(x * x + y * y + z * z);
    nv[0] = x / len; nv[1] = y / len; nv[2] = z / len;
}

__global__ __launch_bounds__(FPFH_WAVE) void normals_kernel(const float* __restrict__ points, const int* __restrict__ n_per_cloud,
                                                            const int* __restrict__ idx, const int* __restrict__ count, int max_nn,
                                                            double vx, double vy, double vz, double* __restrict__ normals, int N) {
    __shared__ int lidx[FPFH_MAX_NN];
    __shared__ double sp[FPFH_MAX_NN][3];            // the list's points in ascending index order
    __shared__ double cum[9];
    const int i = blockIdx.x, b = blockIdx.y, lane = threadIdx.x;
    const int n = cloud_count(n_per_cloud, b, N);
    const size_t row = (size_t)b * N + i;
    double* no = normals + row * 3;
    if (i >= n) {
        if (lane < 3) no[lane] = 0.0;
        return;
    }
    int c = count[row];
    if (c < 0) {
        if (lane < 3) no[lane] = __builtin_nan("");
        return;
    }
    c = c > max_nn ? max_nn : c;
    if (c < 3) {                                     // open3d: no covariance from fewer than 3 neighbours
        if (lane < 3) no[lane] = lane == 2 ? 1.0 : 0.0;
        return;
    }
    const float* pb = points + (size_t)b * N * 3;
    const int* li = idx + row * max_nn;
    for (int e = lane; e < c; e += FPFH_WAVE) lidx[e] = li[e];
    __syncthreads();
    for (int e = lane; e < c; e += FPFH_WAVE) {
        const int id = lidx[e];
        int rank = 0;
        for (int o = 0; o < c; ++o) rank += lidx[o] < id ? 1 : 0;
        const int r = list_row(id, n);
        sp[rank][0] = (double)pb[r * 3];
        sp[rank][1] = (double)pb[r * 3 + 1];
        sp[rank][2] = (double)pb[r * 3 + 2];
    }
    __syncthreads();
    if (lane < 9) {                                  // x y z xx xy xz yy yz zz, each summed in ascending index order
        const int ia = lane < 3 ? lane : (lane < 6 ? 0 : (lane < 8 ? 1 : 2));
        const int ib = lane < 3 ? -1 : (lane < 6 ? lane - 3 : (lane < 8 ? lane - 5 : 2));
        double s = 0.0;
        for (int e = 0; e < c; ++e) {
            const double a = sp[e][ia];
            s += ib < 0 ? a : a * sp[e][ib];
        }
        cum[lane] = s / (double)c;
    }
    __syncthreads();
    if (lane == 0) {
        const double c00 = cum[3] - cum[0] * cum[0], c01 = cum[4] - cum[0] * cum[1], c02 = cum[5] - cum[0] * cum[2];
        const double c11 = cum[6] - cum[1] * cum[1], c12 = cum[7] - cum[1] * cum[2], c22 = cum[8] - cum[2] * cum[2];
        double nv[3];
        smallest_eigenvector(c00, c01, c02, c11, c12, c22, nv);
        const double px = (double)pb[i * 3], py = (double)pb[i * 3 + 1], pz = (double)pb[i * 3 + 2];
        const double d = nv[0] * (vx - px) + nv[1] * (vy - py) + nv[2] * (vz - pz);
        const double sgn = d >= 0.0 ? 1.0 : -1.0;    // NORMAL_SIGN_RULE
        no[0] = sgn * nv[0]; no[1] = sgn * nv[1]; no[2] = sgn * nv[2];
    }
}

// ---- c. SPFH ------------------------------------------------------------------------------------------------------------------
constexpr double FPFH_PI = 3.14159265358979323846;

__device__ __forceinline__ int fpfh_bin(double t) {   // floor, clamped to 0 .. 10 (NaN: 0)
    const double f = floor(t);
    return f >= 0.0 ? (f < 10.0 ? (int)f : 10) : 0;
}

// ComputePairFeatures (open3d 0.9 Feature.cpp), as DESIGN.md f-7 states it
__device__ inline void pair_features(const double (&p1)[3], const double (&n1)[3], const double (&p2)[3], const double (&n2)[3],
                                     double& f1, double& f2, double& f3) {
    f1 = f2 = f3 = 0.0;
    double dp[3] = {p2[0] - p1[0], p2[1] - p1[1], p2[2] - p1[2]};
    const double d = sqrt(dp[0] * dp[0] + dp[1] * dp[1] + dp[2] * dp[2]);
    if (d == 0.0) return;
    const double a1 = (n1[0] * dp[0] + n1[1] * dp[1] + n1[2] * dp[2]) / d;
    const double a2 = (n2[0] * dp[0] + n2[1] * dp[1] + n2[2] * dp[2]) / d;
    const bool swap = acos(fabs(a1)) > acos(fabs(a2));
    double m1[3], m2[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        m1[k] = swap ? n2[k] : n1[k];
        m2[k] = swap ? n1[k] : n2[k];
        dp[k] = swap ? -dp[k] : dp[k];
    }
    double v[3] = {dp[1] * m1[2] - dp[2] * m1[1], dp[2] * m1[0] - dp[0] * m1[2], dp[0] * m1[1] - dp[1] * m1[0]};
    const double vn = sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
    if (vn == 0.0) return;
    v[0] /= vn; v[1] /= vn; v[2] /= vn;
    const double w[3] = {m1[1] * v[2] - m1[2] * v[1], m1[2] * v[0] - m1[0] * v[2], m1[0] * v[1] - m1[1] * v[0]};
    f3 = swap ? -a2 : a1;
    f2 = v[0] * m2[0] + v[1] * m2[1] + v[2] * m2[2];
    f1 = atan2(w[0] * m2[0] + w[1] * m2[1] + w[2] * m2[2], m1[0] * m2[0] + m1[1] * m2[1] + m1[2] * m2[2]);
}

__global__ __launch_bounds__(FPFH_WAVE) void spfh_kernel(const float* __restrict__ points, const int* __restrict__ n_per_cloud,
                                                         const double* __restrict__ normals, const int* __restrict__ idx,
                                                         const int* __restrict__ count, int max_nn, double* __restrict__ spfh, int N) {
    __shared__ int hist[FPFH_DIM];
    const int i = blockIdx.x, b = blockIdx.y, lane = threadIdx.x;
    const int n = cloud_count(n_per_cloud, b, N);
    const size_t row = (size_t)b * N + i;
    double* so = spfh + row * FPFH_DIM;
    if (i >= n) {
        if (lane < FPFH_DIM) so[lane] = 0.0;
        return;
    }
    int c = count[row];
    if (c < 0) {
        if (lane < FPFH_DIM) so[lane] = __builtin_nan("");
        return;
    }
    c = c > max_nn ? max_nn : c;
    if (lane < FPFH_DIM) hist[lane] = 0;
    __syncthreads();
    const float* pb = points + (size_t)b * N * 3;
    const double* nb = normals + (size_t)b * N * 3;
    const int* li = idx + row * max_nn;
    const double p1[3] = {(double)pb[i * 3], (double)pb[i * 3 + 1], (double)pb[i * 3 + 2]};
    const double n1[3] = {nb[i * 3], nb[i * 3 + 1], nb[i * 3 + 2]};
    for (int k = 1 + lane; k < c; k += FPFH_WAVE) {
        const int r = list_row(li[k], n);
        const double p2[3] = {(double)pb[r * 3], (double)pb[r * 3 + 1], (double)pb[r * 3 + 2]};
        const double n2[3] = {nb[r * 3], nb[r * 3 + 1], nb[r * 3 + 2]};
        double f1, f2, f3;
        pair_features(p1, n1, p2, n2, f1, f2, f3);
        atomicAdd(&hist[fpfh_bin(11.0 * (f1 + FPFH_PI) / (2.0 * FPFH_PI))], 1);
        atomicAdd(&hist[11 + fpfh_bin(11.0 * (f2 + 1.0) * 0.5)], 1);
        atomicAdd(&hist[22 + fpfh_bin(11.0 * (f3 + 1.0) * 0.5)], 1);
    }
    __syncthreads();
    if (lane < FPFH_DIM) so[lane] = c > 1 ? (double)hist[lane] * (100.0 / (double)(c - 1)) : 0.0;
}

// ---- d. FPFH ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(FPFH_WAVE) void fpfh_kernel(const double* __restrict__ spfh, const int* __restrict__ n_per_cloud,
                                                         const int* __restrict__ idx, const double* __restrict__ d2,
                                                         const int* __restrict__ count, int max_nn, double* __restrict__ fpfh_f64,
                                                         float* __restrict__ desc_f32, int N) {
    __shared__ int lidx[FPFH_MAX_NN];
    __shared__ double ld2[FPFH_MAX_NN];
    const int i = blockIdx.x, b = blockIdx.y, lane = threadIdx.x;
    const int n = cloud_count(n_per_cloud, b, N);
    const size_t row = (size_t)b * N + i;
    int c = i < n ? count[row] : 0;
    if (i >= n || c < 0) {
        if (lane < FPFH_DIM) {
            if (fpfh_f64) fpfh_f64[row * FPFH_DIM + lane] = i >= n ? 0.0 : __builtin_nan("");
            if (desc_f32) desc_f32[row * FPFH_DIM + lane] = i >= n ? 0.f : __builtin_nanf("");
        }
        return;
    }
    c = c > max_nn ? max_nn : c;
    for (int e = lane; e < c; e += FPFH_WAVE) {
        lidx[e] = list_row(idx[row * max_nn + e], n);
        ld2[e] = d2[row * max_nn + e];
    }
    __syncthreads();
    const double* sb = spfh + (size_t)b * N * FPFH_DIM;
    const int bin = lane < FPFH_DIM ? lane : FPFH_DIM - 1;       // lanes 33 .. 63 shadow the last bin and write nothing
    const int blk = lane < 3 ? lane : 0;                         // lanes 0 .. 2 carry the three block sums
    double f = 0.0, sum = 0.0;
    for (int k = 1; k < c; ++k) {
        const double dist = ld2[k];
        if (dist == 0.0) continue;                               // a duplicate of the point: skipped (open3d)
        const double val = sb[(size_t)lidx[k] * FPFH_DIM + bin] / dist;
        f += val;
#pragma unroll
        for (int j = 0; j < 11; ++j) sum += __shfl(val, blk * 11 + j, 64);       // neighbour-major, bin-minor: ComputeFPFHFeature's order
    }
    const double bsum = __shfl(sum, bin / 11, 64);
    const double scale = bsum != 0.0 ? 100.0 / bsum : 0.0;
    f = f * scale + sb[(size_t)i * FPFH_DIM + bin];
    if (fpfh_f64 && lane < FPFH_DIM) fpfh_f64[row * FPFH_DIM + lane] = f;
    if (desc_f32) {                                              // demo_registration.py:43: f / (|f|_2 + 1e-6)
        const double nrm = sqrt(wave_sum(lane < FPFH_DIM ? f * f : 0.0));
        if (lane < FPFH_DIM) desc_f32[row * FPFH_DIM + lane] = (float)(f / (nrm + 1e-6));
    }
}

// ---- host side ----------------------------------------------------------------------------------------------------------------
struct FpfhLayout {
    size_t nb, idx_n, count_n, idx_f, d2_f, count_f, normals, spfh, bytes;
};

inline FpfhLayout fpfh_layout(int bs, int N, int nn_n, int nn_f) {
    FpfhLayout L;
    const long long rows = (long long)bs * N;
    size_t o = 0;
    L.nb = o;      o += nb_layout(N).cloud_bytes * (size_t)bs;
    L.idx_n = o;   o += (size_t)round_up(rows * nn_n * 4, 256);
    L.count_n = o; o += (size_t)round_up(rows * 4, 256);
    L.idx_f = o;   o += (size_t)round_up(rows * nn_f * 4, 256);
    L.d2_f = o;    o += (size_t)round_up(rows * nn_f * 8, 256);
    L.count_f = o; o += (size_t)round_up(rows * 4, 256);
    L.normals = o; o += (size_t)round_up(rows * 24, 256);
    L.spfh = o;    o += (size_t)round_up(rows * FPFH_DIM * 8, 256);
    L.bytes = o;
    return L;
}

inline bool shape_ok(int bs, int N) { return bs > 0 && bs <= 65535 && N > 0 && N <= (1 << 24); }
inline bool nn_ok(int max_nn) { return max_nn >= 1 && max_nn <= FPFH_MAX_NN; }
inline bool radius_ok(double r) { return r > 0.0 && isfinite(r); }

// the launches of a neighbour search (the grid: one kernel, or the five of path many; then the search); arguments checked by the caller
int enqueue_neighbours(const float* points, const int* n_per_cloud, double radius, int max_nn, int* idx, double* d2, int* count,
                       void* workspace, int bs, int N, int path, hipStream_t st, const char* what) {
    const NbLayout L = nb_layout(N);
    // FLANN's radius search takes the squared radius as float: float(r * r), compared with '<' against the fp64 distance
    const double r2 = (double)(float)(radius * radius);
    unsigned char* ws = (unsigned char*)workspace;
    int rc;
    if (!path_many(path, N)) {
        hipLaunchKernelGGL(nb_grid_kernel, dim3(bs), dim3(ICP_NT), 0, st, points, n_per_cloud, radius, ws, L, N);
        rc = check_launch(what);
        if (rc != PDSC_OK) return rc;
    } else {
        const int nchunk = cloud_chunks(N);
        hipLaunchKernelGGL(cloud_box_kernel, dim3(nchunk, bs), dim3(ICP_NT), 0, st, points, n_per_cloud, ws + L.parts, L.cloud_bytes,
                           ws + L.cells, L.cloud_bytes, icp_hash_size(N) + 1, N);
        rc = check_launch(what);
        if (rc != PDSC_OK) return rc;
        hipLaunchKernelGGL(nb_header_kernel, dim3(bs), dim3(ICP_NT), 0, st, n_per_cloud, radius, ws, L, N);
        rc = check_launch(what);
        if (rc != PDSC_OK) return rc;
        hipLaunchKernelGGL(nb_hist_kernel, dim3(nchunk, bs), dim3(ICP_NT), 0, st, points, n_per_cloud, ws, L, N);
        rc = check_launch(what);
        if (rc != PDSC_OK) return rc;
        hipLaunchKernelGGL(nb_scan_kernel, dim3(bs), dim3(ICP_NT), 0, st, ws, L);
        rc = check_launch(what);
        if (rc != PDSC_OK) return rc;
        hipLaunchKernelGGL(nb_scatter_kernel, dim3(nchunk, bs), dim3(ICP_NT), 0, st, points, n_per_cloud, ws, L, N);
        rc = check_launch(what);
        if (rc != PDSC_OK) return rc;
    }
    hipLaunchKernelGGL(nb_search_kernel, dim3(N, bs), dim3(FPFH_WAVE), 0, st, points, n_per_cloud, r2, max_nn, idx, d2, count,
                       (const unsigned char*)workspace, L, N);
    return check_launch(what);
}

}  // namespace

size_t hybrid_neighbours_workspace_bytes(int bs, int N) {
    if (!shape_ok(bs, N)) return 0;
    return nb_layout(N).cloud_bytes * (size_t)bs;
}

size_t fpfh_workspace_bytes(int bs, int N, int nn_n, int nn_f) {
    if (!shape_ok(bs, N) || !nn_ok(nn_n) || !nn_ok(nn_f)) return 0;
    return fpfh_layout(bs, N, nn_n, nn_f).bytes;
}

int launch_hybrid_neighbours(const float* points, const int* n_per_cloud, double radius, int max_nn, int* idx, double* d2, int* count,
                             void* workspace, size_t workspace_bytes, int bs, int N, int path, hipStream_t st) {
    PDSC_REQUIRE(points && idx && count && workspace, "pdsc_hybrid_neighbours: null pointer");
    PDSC_REQUIRE(shape_ok(bs, N), "pdsc_hybrid_neighbours: bs=%d N=%d", bs, N);
    PDSC_REQUIRE(radius_ok(radius), "pdsc_hybrid_neighbours: radius %g must be positive and finite", radius);
    PDSC_REQUIRE(nn_ok(max_nn), "pdsc_hybrid_neighbours: max_nn=%d outside 1 .. %d", max_nn, FPFH_MAX_NN);
    PDSC_REQUIRE(path_ok(path), "pdsc_hybrid_neighbours: path=%d outside 0 .. 2", path);
    const size_t need = hybrid_neighbours_workspace_bytes(bs, N);
    PDSC_REQUIRE(workspace_bytes >= need, "pdsc_hybrid_neighbours: workspace %zu bytes < %zu", workspace_bytes, need);
    return enqueue_neighbours(points, n_per_cloud, radius, max_nn, idx, d2, count, workspace, bs, N, path, st, "pdsc_hybrid_neighbours");
}

int launch_estimate_normals(const float* points, const int* n_per_cloud, const int* idx, const int* count, int max_nn,
                            const double* viewpoint, double* normals, int bs, int N, hipStream_t st) {
    PDSC_REQUIRE(points && idx && count && normals, "pdsc_estimate_normals: null pointer");
    PDSC_REQUIRE(shape_ok(bs, N), "pdsc_estimate_normals: bs=%d N=%d", bs, N);
    PDSC_REQUIRE(nn_ok(max_nn), "pdsc_estimate_normals: max_nn=%d outside 1 .. %d", max_nn, FPFH_MAX_NN);
    const double vx = viewpoint ? viewpoint[0] : 0.0, vy = viewpoint ? viewpoint[1] : 0.0, vz = viewpoint ? viewpoint[2] : 0.0;
    PDSC_REQUIRE(isfinite(vx) && isfinite(vy) && isfinite(vz), "pdsc_estimate_normals: viewpoint is not finite");
    hipLaunchKernelGGL(normals_kernel, dim3(N, bs), dim3(FPFH_WAVE), 0, st, points, n_per_cloud, idx, count, max_nn, vx, vy, vz, normals,
                       N);
    return check_launch("pdsc_estimate_normals");
}

int launch_spfh(const float* points, const int* n_per_cloud, const double* normals, const int* idx, const int* count, int max_nn,
                double* spfh, int bs, int N, hipStream_t st) {
    PDSC_REQUIRE(points && normals && idx && count && spfh, "pdsc_spfh: null pointer");
    PDSC_REQUIRE(shape_ok(bs, N), "pdsc_spfh: bs=%d N=%d", bs, N);
    PDSC_REQUIRE(nn_ok(max_nn), "pdsc_spfh: max_nn=%d outside 1 .. %d", max_nn, FPFH_MAX_NN);
    hipLaunchKernelGGL(spfh_kernel, dim3(N, bs), dim3(FPFH_WAVE), 0, st, points, n_per_cloud, normals, idx, count, max_nn, spfh, N);
    return check_launch("pdsc_spfh");
}

int launch_fpfh_from_spfh(const double* spfh, const int* n_per_cloud, const int* idx, const double* d2, const int* count, int max_nn,
                          double* fpfh_f64, float* desc_f32, int bs, int N, hipStream_t st) {
    PDSC_REQUIRE(spfh && idx && d2 && count && (fpfh_f64 || desc_f32), "pdsc_fpfh_from_spfh: null pointer");
    PDSC_REQUIRE(shape_ok(bs, N), "pdsc_fpfh_from_spfh: bs=%d N=%d", bs, N);
    PDSC_REQUIRE(nn_ok(max_nn), "pdsc_fpfh_from_spfh: max_nn=%d outside 1 .. %d", max_nn, FPFH_MAX_NN);
    hipLaunchKernelGGL(fpfh_kernel, dim3(N, bs), dim3(FPFH_WAVE), 0, st, spfh, n_per_cloud, idx, d2, count, max_nn, fpfh_f64, desc_f32,
                       N);
    return check_launch("pdsc_fpfh_from_spfh");
}

int launch_fpfh(const float* points, const int* n_per_cloud, double normal_radius, int normal_max_nn, double feature_radius,
                int feature_max_nn, const double* viewpoint, double* fpfh_f64, float* desc_f32, double* normals_out, void* workspace,
                size_t workspace_bytes, int bs, int N, hipStream_t st) {
    // everything is checked before the first launch: a refused call enqueues nothing
    PDSC_REQUIRE(points && (fpfh_f64 || desc_f32) && workspace, "pdsc_fpfh: null pointer");
    PDSC_REQUIRE(shape_ok(bs, N), "pdsc_fpfh: bs=%d N=%d", bs, N);
    PDSC_REQUIRE(radius_ok(normal_radius) && radius_ok(feature_radius), "pdsc_fpfh: radii %g / %g must be positive and finite",
                 normal_radius, feature_radius);
    PDSC_REQUIRE(nn_ok(normal_max_nn) && nn_ok(feature_max_nn), "pdsc_fpfh: max_nn=%d / %d outside 1 .. %d", normal_max_nn,
                 feature_max_nn, FPFH_MAX_NN);
    PDSC_REQUIRE(!viewpoint || (isfinite(viewpoint[0]) && isfinite(viewpoint[1]) && isfinite(viewpoint[2])),
                 "pdsc_fpfh: viewpoint is not finite");
    const FpfhLayout L = fpfh_layout(bs, N, normal_max_nn, feature_max_nn);
    PDSC_REQUIRE(workspace_bytes >= L.bytes, "pdsc_fpfh: workspace %zu bytes < %zu", workspace_bytes, L.bytes);
    unsigned char* ws = (unsigned char*)workspace;
    int* idx_n = reinterpret_cast<int*>(ws + L.idx_n);
    int* count_n = reinterpret_cast<int*>(ws + L.count_n);
    int* idx_f = reinterpret_cast<int*>(ws + L.idx_f);
    double* d2_f = reinterpret_cast<double*>(ws + L.d2_f);
    int* count_f = reinterpret_cast<int*>(ws + L.count_f);
    double* normals = normals_out ? normals_out : reinterpret_cast<double*>(ws + L.normals);
    double* spfh = reinterpret_cast<double*>(ws + L.spfh);
    int rc = enqueue_neighbours(points, n_per_cloud, normal_radius, normal_max_nn, idx_n, nullptr, count_n, ws + L.nb, bs, N,
                                PDSC_PATH_AUTO, st,
                                "pdsc_fpfh");
    if (rc != PDSC_OK) return rc;
    rc = launch_estimate_normals(points, n_per_cloud, idx_n, count_n, normal_max_nn, viewpoint, normals, bs, N, st);
    if (rc != PDSC_OK) return rc;
    rc = enqueue_neighbours(points, n_per_cloud, feature_radius, feature_max_nn, idx_f, d2_f, count_f, ws + L.nb, bs, N, PDSC_PATH_AUTO, st,
                            "pdsc_fpfh");
    if (rc != PDSC_OK) return rc;
    rc = launch_spfh(points, n_per_cloud, normals, idx_f, count_f, feature_max_nn, spfh, bs, N, st);
    if (rc != PDSC_OK) return rc;
    return launch_fpfh_from_spfh(spfh, n_per_cloud, idx_f, d2_f, count_f, feature_max_nn, fpfh_f64, desc_f32, bs, N, st);
}

}  // namespace pdsc

extern "C" size_t pdsc_hybrid_neighbours_workspace_bytes(int bs, int N) { return pdsc::hybrid_neighbours_workspace_bytes(bs, N); }

extern "C" int pdsc_hybrid_neighbours(const float* points, const int* n_per_cloud, double radius, int max_nn, int* idx, double* d2,
                                      int* count, void* workspace, size_t workspace_bytes, int bs, int N, void* stream) {
    return pdsc::launch_hybrid_neighbours(points, n_per_cloud, radius, max_nn, idx, d2, count, workspace, workspace_bytes, bs, N,
                                          PDSC_PATH_AUTO, (hipStream_t)stream);
}

extern "C" int pdsc_cloud_neighbours(const float* points, const int* n_per_cloud, double radius, int max_nn, int* idx, double* d2,
                                     int* count, void* workspace, size_t workspace_bytes, int bs, int N, int path, void* stream) {
    return pdsc::launch_hybrid_neighbours(points, n_per_cloud, radius, max_nn, idx, d2, count, workspace, workspace_bytes, bs, N, path,
                                          (hipStream_t)stream);
}

extern "C" int pdsc_estimate_normals(const float* points, const int* n_per_cloud, const int* idx, const int* count, int max_nn,
                                     const double* viewpoint, double* normals, int bs, int N, void* stream) {
    return pdsc::launch_estimate_normals(points, n_per_cloud, idx, count, max_nn, viewpoint, normals, bs, N, (hipStream_t)stream);
}

extern "C" int pdsc_spfh(const float* points, const int* n_per_cloud, const double* normals, const int* idx, const int* count,
                         int max_nn, double* spfh, int bs, int N, void* stream) {
    return pdsc::launch_spfh(points, n_per_cloud, normals, idx, count, max_nn, spfh, bs, N, (hipStream_t)stream);
}

extern "C" int pdsc_fpfh_from_spfh(const double* spfh, const int* n_per_cloud, const int* idx, const double* d2, const int* count,
                                   int max_nn, double* fpfh_f64, float* desc_f32, int bs, int N, void* stream) {
    return pdsc::launch_fpfh_from_spfh(spfh, n_per_cloud, idx, d2, count, max_nn, fpfh_f64, desc_f32, bs, N, (hipStream_t)stream);
}

extern "C" size_t pdsc_fpfh_workspace_bytes(int bs, int N, int normal_max_nn, int feature_max_nn) {
    return pdsc::fpfh_workspace_bytes(bs, N, normal_max_nn, feature_max_nn);
}

extern "C" int pdsc_fpfh(const float* points, const int* n_per_cloud, double normal_radius, int normal_max_nn, double feature_radius,
                         int feature_max_nn, const double* viewpoint, double* fpfh_f64, float* desc_f32, double* normals_out,
                         void* workspace, size_t workspace_bytes, int bs, int N, void* stream) {
    return pdsc::launch_fpfh(points, n_per_cloud, normal_radius, normal_max_nn, feature_radius, feature_max_nn, viewpoint, fpfh_f64,
                             desc_f32, normals_out, workspace, workspace_bytes, bs, N, (hipStream_t)stream);
}
