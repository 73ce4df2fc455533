// f-6: open3d PointCloud.voxel_down_sample for the multiway driver's multi_scale_icp (multiway/test_multi_ate.py:58-59), on the
// device, as harness.voxel_down_sample restates it: grid anchored at min - voxel / 2, fp64 floor((p - origin) / voxel) per axis,
// one output point per occupied voxel = the fp64 mean of its points rounded to fp32, output ordered by ascending voxel index
// (ix dy + iy) dz + iz, the points of a voxel summed in input order.
// Two kernels around a stable sort of the keys (the caller's: torch.sort(stable=True) in the Python wrapper):
//   voxel_keys_kernel   one 512-thread workgroup per cloud: bounds (fp32 min / max: exact), then one int64 key per point;
//   voxel_means_kernel  one 512-thread workgroup per cloud walks the sorted keys in tiles of 512: a ballot scan numbers the runs
//                       of equal keys, the thread at the head of a run sums it sequentially (fp64, sorted = input order).
// Bound: latency (one workgroup per cloud, gathers through the permutation); reported as time only.  Known limit: a run is summed
// by ONE thread, also across tiles, in a chain of dependent gathers -- the order the contract fixes (input order) -- so the time has
// a term of (points in the fullest voxel) sequential loads; with a voxel much coarser than the point spacing (in the worst case one
// voxel holds the cloud) the other 511 threads wait for it.  The driver's scales keep runs short (tens of points at 0.05 m on
// the dense test cloud).  Splitting a long run would need partial sums in another association than input order.
#include "icp_grid.h"

namespace pdsc {
namespace {

constexpr long long VOXEL_PAD_KEY = 0x7FFFFFFFFFFFFFFFll;    // INT64_MAX: padding rows, and every row of a cloud without a grid
// voxels per axis: the key (ix dy + iy) dz + iz stays below 2^60
constexpr double VOXEL_MAX_PER_AXIS = 1048576.0;

__global__ __launch_bounds__(ICP_NT) void voxel_keys_kernel(const float* __restrict__ points, const int* __restrict__ n_per_cloud,
                                                            double voxel, long long* __restrict__ keys, int N) {
    __shared__ float bb[ICP_NW * 6];
    const int b = blockIdx.x, t = threadIdx.x;
    int n = n_per_cloud ? n_per_cloud[b] : N;
    n = n < 0 ? 0 : (n > N ? N : n);
    const float* pb = points + (size_t)b * N * 3;
    long long* kb = keys + (size_t)b * N;

    float mn[3], mx[3];
    const bool bad = cloud_bounds(pb, n, mn, mx);
    const bool any_bad = __syncthreads_or(bad);
    block_bounds(mn, mx, bb);
    float lo[3], hi[3];
    block_bounds_read(bb, lo, hi);
    double origin[3], dims[3];
    bool grid_ok = !any_bad && n > 0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        origin[k] = (double)lo[k] - 0.5 * voxel;
        // floor((p - origin) / voxel) is monotone in p: the largest index of an axis is that of the largest coordinate
        dims[k] = floor(((double)hi[k] - origin[k]) / voxel) + 1.0;
        grid_ok = grid_ok && dims[k] >= 1.0 && dims[k] <= VOXEL_MAX_PER_AXIS;
    }
    // a non-finite point, an empty cloud or a grid beyond 2^20 voxels per axis: no key, the cloud down-samples to 0 points
    const long long dy = grid_ok ? (long long)dims[1] : 0, dz = grid_ok ? (long long)dims[2] : 0;
    for (int i = t; i < N; i += ICP_NT) {
        long long key = VOXEL_PAD_KEY;
        if (grid_ok && i < n) {
            const long long ix = (long long)floor(((double)pb[i * 3] - origin[0]) / voxel);
            const long long iy = (long long)floor(((double)pb[i * 3 + 1] - origin[1]) / voxel);
            const long long iz = (long long)floor(((double)pb[i * 3 + 2] - origin[2]) / voxel);
            key = (ix * dy + iy) * dz + iz;
        }
        kb[i] = key;
    }
}

__global__ __launch_bounds__(ICP_NT) void voxel_means_kernel(const float* __restrict__ points, const long long* __restrict__ sorted_keys,
                                                             const long long* __restrict__ perm, float* __restrict__ out,
                                                             int* __restrict__ counts, int N) {
    __shared__ int wtot[ICP_NW];
    const int b = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const float* pb = points + (size_t)b * N * 3;
    const long long* kb = sorted_keys + (size_t)b * N;
    const long long* qb = perm + (size_t)b * N;
    float* ob = out + (size_t)b * N * 3;

    int base = 0;                                                    // runs before this tile (the same in every thread)
    for (int tile = 0; tile < N; tile += ICP_NT) {
        if (kb[tile] == VOXEL_PAD_KEY) break;                        // sorted: everything from here on is padding
        const int i = tile + t;
        const long long key = i < N ? kb[i] : VOXEL_PAD_KEY;
        const bool head = key != VOXEL_PAD_KEY && (i == 0 || kb[i - 1] != key);
        const unsigned long long heads = __ballot(head);
        if (lane == 0) wtot[wave] = __popcll(heads);
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < ICP_NW; ++w) {
            before += w < wave ? wtot[w] : 0;
            total += wtot[w];
        }
        if (head) {
            const int row = base + before + __popcll(heads & ((1ull << lane) - 1ull));
            double sx = 0.0, sy = 0.0, sz = 0.0;
            int cnt = 0;
            for (int j = i; j < N && kb[j] == key; ++j) {
                const long long p = qb[j];
                if (p < 0 || p >= N) continue;                       // not a permutation of 0 .. N-1: never read outside the cloud (an empty run: NaN)
                sx += (double)pb[p * 3]; sy += (double)pb[p * 3 + 1]; sz += (double)pb[p * 3 + 2];
                ++cnt;
            }
            const double c = (double)cnt;
            ob[row * 3] = (float)(sx / c); ob[row * 3 + 1] = (float)(sy / c); ob[row * 3 + 2] = (float)(sz / c);
        }
        base += total;
        __syncthreads();                                             // wtot is rewritten by the next tile
    }
    for (int i = base * 3 + t; i < N * 3; i += ICP_NT) ob[i] = 0.f;  // capacity = input rows: the rest is zero padding
    if (t == 0) counts[b] = base;
}

}  // namespace

int launch_voxel_keys(const float* points, const int* n_per_cloud, double voxel, long long* keys, int bs, int N, hipStream_t st) {
    PDSC_REQUIRE(points && keys, "pdsc_voxel_keys: null pointer");
    PDSC_REQUIRE(bs > 0 && N > 0 && N <= (1 << 24), "pdsc_voxel_keys: bs=%d N=%d", bs, N);
    PDSC_REQUIRE(voxel > 0.0 && isfinite(voxel), "pdsc_voxel_keys: voxel size %g must be positive and finite", voxel);
    hipLaunchKernelGGL(voxel_keys_kernel, dim3(bs), dim3(ICP_NT), 0, st, points, n_per_cloud, voxel, keys, N);
    return check_launch("pdsc_voxel_keys");
}

int launch_voxel_means(const float* points, const long long* sorted_keys, const long long* perm, float* out, int* counts, int bs, int N,
                       hipStream_t st) {
    PDSC_REQUIRE(points && sorted_keys && perm && out && counts, "pdsc_voxel_means: null pointer");
    PDSC_REQUIRE(bs > 0 && N > 0 && N <= (1 << 24), "pdsc_voxel_means: bs=%d N=%d", bs, N);
    hipLaunchKernelGGL(voxel_means_kernel, dim3(bs), dim3(ICP_NT), 0, st, points, sorted_keys, perm, out, counts, N);
    return check_launch("pdsc_voxel_means");
}

}  // namespace pdsc

extern "C" int pdsc_voxel_keys(const float* points, const int* n_per_cloud, double voxel_size, long long* keys, int bs, int N,
                               void* stream) {
    return pdsc::launch_voxel_keys(points, n_per_cloud, voxel_size, keys, bs, N, (hipStream_t)stream);
}

extern "C" int pdsc_voxel_means(const float* points, const long long* sorted_keys, const long long* perm, float* out, int* counts,
                                int bs, int N, void* stream) {
    return pdsc::launch_voxel_means(points, sorted_keys, perm, out, counts, bs, N, (hipStream_t)stream);
}
