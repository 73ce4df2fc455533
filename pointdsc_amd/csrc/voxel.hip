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
//
// f-9 (pdsc_cloud_voxel_keys / pdsc_cloud_voxel_means): the same keys and the same sums for a RAW cloud on its way to the FPFH
// descriptor -- the run's fp64 mean NORMAL beside its mean point (VOXEL_NORMAL_RULE), out_capacity output rows per cloud
// (CAPACITY_RULE), and a path selector: the two kernels above, or short chains of many-workgroup kernels (cloud_many.h):
//   cloud_box_kernel -> voxel_box_kernel -> voxel_keys_many_kernel       per-chunk boxes, their reduction, one key per point;
//   voxel_heads_kernel -> voxel_scan_kernel -> voxel_means_many_kernel   run heads per tile of 512, exclusive scan, the means.
// Bit-identical to the one-workgroup path: min / max are order-free, a key depends on its point and the box alone, a run is still
// summed by the one thread at its head in input order (across tiles and workgroups), and the row of a run is the number of heads
// before it either way.  No kernel waits for another workgroup.
#include "cloud_many.h"

namespace pdsc {
namespace {

constexpr long long VOXEL_PAD_KEY = 0x7FFFFFFFFFFFFFFFll;    // INT64_MAX: padding rows, and every row of a cloud without a grid
// voxels per axis: the key (ix dy + iy) dz + iz stays below 2^60
constexpr double VOXEL_MAX_PER_AXIS = 1048576.0;

struct VoxelGrid {
    double origin[3];
    long long dy, dz;
    bool ok;
};

// the grid of a cloud from its box; a non-finite point, an empty cloud or a grid beyond 2^20 voxels per axis: no grid, no key,
// the cloud down-samples to 0 points
__device__ __forceinline__ VoxelGrid voxel_grid(const float (&lo)[3], const float (&hi)[3], bool any_bad, int n, double voxel) {
    VoxelGrid g;
    double dims[3];
    g.ok = !any_bad && n > 0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        g.origin[k] = (double)lo[k] - 0.5 * voxel;
        // floor((p - origin) / voxel) is monotone in p: the largest index of an axis is that of the largest coordinate
        dims[k] = floor(((double)hi[k] - g.origin[k]) / voxel) + 1.0;
        g.ok = g.ok && dims[k] >= 1.0 && dims[k] <= VOXEL_MAX_PER_AXIS;
    }
    g.dy = g.ok ? (long long)dims[1] : 0;
    g.dz = g.ok ? (long long)dims[2] : 0;
    return g;
}

__device__ __forceinline__ long long voxel_key(const float* __restrict__ pb, int i, int n, const VoxelGrid& g, double voxel) {
    if (!(g.ok && i < n)) return VOXEL_PAD_KEY;
    const long long ix = (long long)floor(((double)pb[i * 3] - g.origin[0]) / voxel);
    const long long iy = (long long)floor(((double)pb[i * 3 + 1] - g.origin[1]) / voxel);
    const long long iz = (long long)floor(((double)pb[i * 3 + 2] - g.origin[2]) / voxel);
    return (ix * g.dy + iy) * g.dz + iz;
}

__global__ __launch_bounds__(ICP_NT) void voxel_keys_kernel(const float* __restrict__ points, const int* __restrict__ n_per_cloud,
                                                            double voxel, long long* __restrict__ keys, int N) {
    __shared__ float bb[ICP_NW * 6];
    const int b = blockIdx.x, t = threadIdx.x;
    const int n = cloud_count(n_per_cloud, b, N);
    const float* pb = points + (size_t)b * N * 3;
    long long* kb = keys + (size_t)b * N;

    float mn[3], mx[3];
    const bool bad = cloud_bounds(pb, n, mn, mx);
    const bool any_bad = __syncthreads_or(bad);
    block_bounds(mn, mx, bb);
    float lo[3], hi[3];
    block_bounds_read(bb, lo, hi);
    const VoxelGrid g = voxel_grid(lo, hi, any_bad, n, voxel);
    for (int i = t; i < N; i += ICP_NT) kb[i] = voxel_key(pb, i, n, g, voxel);
}

// ---- many workgroups: keys ----------------------------------------------------------------------------------------------------
// one workgroup per cloud reduces the chunks' boxes -> box [bs]
__global__ __launch_bounds__(ICP_NT) void voxel_box_kernel(const CloudBox* __restrict__ parts, CloudBox* __restrict__ box, int nchunk) {
    __shared__ float bb[ICP_NW * 6];
    const int b = blockIdx.x;
    float mn[3], mx[3];
    const bool bad = cloud_box_share(parts + (size_t)b * nchunk, nchunk, mn, mx);
    const int any_bad = __syncthreads_or(bad);
    block_bounds(mn, mx, bb);
    if (threadIdx.x == 0) {
        CloudBox o;
        block_bounds_read(bb, o.lo, o.hi);
        o.bad = any_bad ? 1 : 0;
        o.pad_ = 0;
        box[b] = o;
    }
}

// grid (nchunk, bs)
__global__ __launch_bounds__(ICP_NT) void voxel_keys_many_kernel(const float* __restrict__ points, const int* __restrict__ n_per_cloud,
                                                                 const CloudBox* __restrict__ box, double voxel,
                                                                 long long* __restrict__ keys, int N) {
    const int c = blockIdx.x, b = blockIdx.y, t = threadIdx.x;
    const int n = cloud_count(n_per_cloud, b, N);
    const float* pb = points + (size_t)b * N * 3;
    long long* kb = keys + (size_t)b * N;
    const CloudBox bx = box[b];
    const VoxelGrid g = voxel_grid(bx.lo, bx.hi, bx.bad != 0, n, voxel);
    const int i1 = min((c + 1) * CLOUD_CHUNK, N);
    for (int i = c * CLOUD_CHUNK + t; i < i1; i += ICP_NT) kb[i] = voxel_key(pb, i, n, g, voxel);
}

// ---- means ------------------------------------------------------------------------------------------------------------------
struct VoxelMeansArgs {
    const float* points;           // [bs][N][3]
    const double* normals;         // [bs][N][3] (NORMALS only)
    const long long* sorted_keys;  // [bs][N]
    const long long* perm;         // [bs][N]
    float* out;                    // [bs][cap][3]
    double* out_normals;           // [bs][cap][3] (NORMALS only)
    int* counts;                   // [bs]
    int N, cap, renormalize;
};

// the thread at the head i of a run of `key` sums it sequentially in sorted (= input) order and writes output row `row` (< cap)
template <bool NORMALS>
__device__ __forceinline__ void voxel_sum_run(const VoxelMeansArgs& a, int b, int i, long long key, int row) {
    const int N = a.N;
    const float* pb = a.points + (size_t)b * N * 3;
    const long long* kb = a.sorted_keys + (size_t)b * N;
    const long long* qb = a.perm + (size_t)b * N;
    double sx = 0.0, sy = 0.0, sz = 0.0, nx = 0.0, ny = 0.0, nz = 0.0;
    int cnt = 0;
    for (int j = i; j < N && kb[j] == key; ++j) {
        const long long p = qb[j];
        if (p < 0 || p >= N) continue;                       // not a permutation of 0 .. N-1: never read outside the cloud (an empty run: NaN)
        sx += (double)pb[p * 3]; sy += (double)pb[p * 3 + 1]; sz += (double)pb[p * 3 + 2];
        if (NORMALS) {
            const double* nb = a.normals + (size_t)b * N * 3;
            nx += nb[p * 3]; ny += nb[p * 3 + 1]; nz += nb[p * 3 + 2];
        }
        ++cnt;
    }
    const double c = (double)cnt;
    float* ob = a.out + ((size_t)b * a.cap + row) * 3;
    ob[0] = (float)(sx / c); ob[1] = (float)(sy / c); ob[2] = (float)(sz / c);
    if (NORMALS) {
        nx = nx / c; ny = ny / c; nz = nz / c;               // VOXEL_NORMAL_RULE: the mean, not renormalised ...
        if (a.renormalize) {                                 // ... unless asked for; a zero mean stays (0, 0, 0)
            const double len = sqrt((nx * nx + ny * ny) + nz * nz);
            if (len > 0.0) { nx = nx / len; ny = ny / len; nz = nz / len; }
        }
        double* on = a.out_normals + ((size_t)b * a.cap + row) * 3;
        on[0] = nx; on[1] = ny; on[2] = nz;
    }
}

template <bool NORMALS>
__device__ __forceinline__ void voxel_zero_row(const VoxelMeansArgs& a, int b, int row) {
    float* ob = a.out + ((size_t)b * a.cap + row) * 3;
    ob[0] = ob[1] = ob[2] = 0.f;
    if (NORMALS) {
        double* on = a.out_normals + ((size_t)b * a.cap + row) * 3;
        on[0] = on[1] = on[2] = 0.0;
    }
}

// The heads of the tile of ICP_NT sorted keys that starts at `tile`: whether this thread's key starts a run, the heads of the tile
// before this thread, and those of the whole tile.  wtot: ICP_NW ints of LDS; the caller synchronises before the next call.
__device__ __forceinline__ bool voxel_tile_heads(const long long* __restrict__ kb, int tile, int N, int* wtot, long long& key,
                                                 int& before, int& total) {
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int i = tile + t;
    key = i < N ? kb[i] : VOXEL_PAD_KEY;
    const bool head = key != VOXEL_PAD_KEY && (i == 0 || kb[i - 1] != key);
    const unsigned long long heads = __ballot(head);
    if (lane == 0) wtot[wave] = __popcll(heads);
    __syncthreads();
    before = 0;
    total = 0;
#pragma unroll
    for (int w = 0; w < ICP_NW; ++w) {
        before += w < wave ? wtot[w] : 0;
        total += wtot[w];
    }
    before += __popcll(heads & ((1ull << lane) - 1ull));
    return head;
}

template <bool NORMALS>
__global__ __launch_bounds__(ICP_NT) void voxel_means_kernel(VoxelMeansArgs a) {
    __shared__ int wtot[ICP_NW];
    const int b = blockIdx.x, t = threadIdx.x, N = a.N;
    const long long* kb = a.sorted_keys + (size_t)b * N;

    int base = 0;                                                    // runs before this tile (the same in every thread)
    for (int tile = 0; tile < N; tile += ICP_NT) {
        if (kb[tile] == VOXEL_PAD_KEY) break;                        // sorted: everything from here on is padding
        long long key;
        int before, total;
        const bool head = voxel_tile_heads(kb, tile, N, wtot, key, before, total);
        if (head && base + before < a.cap) voxel_sum_run<NORMALS>(a, b, tile + t, key, base + before);
        base += total;
        __syncthreads();                                             // wtot is rewritten by the next tile
    }
    const bool over = base > a.cap;                                  // CAPACITY_RULE: count -1 and zero rows
    for (int r = (over ? 0 : base) + t; r < a.cap; r += ICP_NT) voxel_zero_row<NORMALS>(a, b, r);
    if (t == 0) a.counts[b] = over ? -1 : base;
}

// grid (ntile, bs): the number of run heads in tile blockIdx.x -> heads [bs][ntile + 1]
__global__ __launch_bounds__(ICP_NT) void voxel_heads_kernel(const long long* __restrict__ sorted_keys, int* __restrict__ heads, int N) {
    const int tile = blockIdx.x, ntile = gridDim.x, b = blockIdx.y;
    const long long* kb = sorted_keys + (size_t)b * N;
    const int i = tile * ICP_NT + threadIdx.x;
    const long long key = i < N ? kb[i] : VOXEL_PAD_KEY;
    const bool head = key != VOXEL_PAD_KEY && (i == 0 || kb[i - 1] != key);
    const int cnt = __syncthreads_count(head);
    if (threadIdx.x == 0) heads[(size_t)b * (ntile + 1) + tile] = cnt;
}

// one workgroup per cloud: heads [ntile] -> its exclusive scan, heads[ntile] = the number of runs; counts[b] under CAPACITY_RULE
__global__ __launch_bounds__(ICP_NT) void voxel_scan_kernel(int* __restrict__ heads, int* __restrict__ counts, int ntile, int cap) {
    __shared__ int scan[ICP_NT];
    const int b = blockIdx.x, t = threadIdx.x;
    int* hb = heads + (size_t)b * (ntile + 1);
    const int per = (ntile + ICP_NT - 1) / ICP_NT;
    const int h0 = min(t * per, ntile), h1 = min(h0 + per, ntile);
    int local = 0;
    for (int h = h0; h < h1; ++h) local += hb[h];
    scan[t] = local;
    __syncthreads();
    for (int off = 1; off < ICP_NT; off <<= 1) {
        const int v = scan[t] + (t >= off ? scan[t - off] : 0);
        __syncthreads();
        scan[t] = v;
        __syncthreads();
    }
    int run = scan[t] - local;
    for (int h = h0; h < h1; ++h) {
        const int c = hb[h];
        hb[h] = run;
        run += c;
    }
    if (t == ICP_NT - 1) {
        const int total = scan[t];
        hb[ntile] = total;
        counts[b] = total > cap ? -1 : total;
    }
}

// grid (ntile, bs): tile blockIdx.x of the one-workgroup kernel's loop, its `base` read from the scan
template <bool NORMALS>
__global__ __launch_bounds__(ICP_NT) void voxel_means_many_kernel(VoxelMeansArgs a, const int* __restrict__ heads) {
    __shared__ int wtot[ICP_NW];
    const int tile = blockIdx.x, ntile = gridDim.x, b = blockIdx.y, t = threadIdx.x, N = a.N;
    const long long* kb = a.sorted_keys + (size_t)b * N;
    const int* hb = heads + (size_t)b * (ntile + 1);
    const int base = hb[tile], runs = hb[ntile];
    const bool over = runs > a.cap;
    long long key;
    int before, total;
    const bool head = voxel_tile_heads(kb, tile * ICP_NT, N, wtot, key, before, total);
    if (head && !over) voxel_sum_run<NORMALS>(a, b, tile * ICP_NT + t, key, base + before);   // base + before < runs <= cap
    // the rows that no run writes: this workgroup's share of them
    for (int r = tile * ICP_NT + t; r < a.cap; r += ntile * ICP_NT) {
        if (over || r >= runs) voxel_zero_row<NORMALS>(a, b, r);
    }
}

// the workspace is region-major: the chunk boxes of all clouds, then their reduced boxes, then their head counts
struct VoxelLayout {
    size_t parts, box, heads, bytes;
};

inline VoxelLayout voxel_layout(int bs, int N) {
    VoxelLayout L;
    size_t o = 0;
    L.parts = o; o += (size_t)round_up((long long)bs * cloud_chunks(N) * (long long)sizeof(CloudBox), 256);
    L.box = o;   o += (size_t)round_up((long long)bs * (long long)sizeof(CloudBox), 256);
    L.heads = o; o += (size_t)round_up((long long)bs * (ceil_div(N, ICP_NT) + 1) * 4, 256);
    L.bytes = o;
    return L;
}

inline bool voxel_shape_ok(int bs, int N) { return bs > 0 && bs <= 65535 && N > 0 && N <= (1 << 24); }

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
    const VoxelMeansArgs a{points, nullptr, sorted_keys, perm, out, nullptr, counts, N, N, 0};
    hipLaunchKernelGGL(voxel_means_kernel<false>, dim3(bs), dim3(ICP_NT), 0, st, a);
    return check_launch("pdsc_voxel_means");
}

size_t cloud_voxel_workspace_bytes(int bs, int N) {
    if (!voxel_shape_ok(bs, N)) return 0;
    return voxel_layout(bs, N).bytes;
}

int launch_cloud_voxel_keys(const float* points, const int* n_per_cloud, double voxel, long long* keys, void* workspace,
                            size_t workspace_bytes, int bs, int N, int path, hipStream_t st) {
    PDSC_REQUIRE(points && keys && workspace, "pdsc_cloud_voxel_keys: null pointer");
    PDSC_REQUIRE(voxel_shape_ok(bs, N), "pdsc_cloud_voxel_keys: bs=%d N=%d", bs, N);
    PDSC_REQUIRE(voxel > 0.0 && isfinite(voxel), "pdsc_cloud_voxel_keys: voxel size %g must be positive and finite", voxel);
    PDSC_REQUIRE(path_ok(path), "pdsc_cloud_voxel_keys: path=%d outside 0 .. 2", path);
    const VoxelLayout L = voxel_layout(bs, N);
    PDSC_REQUIRE(workspace_bytes >= L.bytes, "pdsc_cloud_voxel_keys: workspace %zu bytes < %zu", workspace_bytes, L.bytes);
    if (!path_many(path, N)) {
        hipLaunchKernelGGL(voxel_keys_kernel, dim3(bs), dim3(ICP_NT), 0, st, points, n_per_cloud, voxel, keys, N);
        return check_launch("pdsc_cloud_voxel_keys");
    }
    unsigned char* ws = (unsigned char*)workspace;
    CloudBox* parts = reinterpret_cast<CloudBox*>(ws + L.parts);
    CloudBox* box = reinterpret_cast<CloudBox*>(ws + L.box);
    const int nchunk = cloud_chunks(N);
    hipLaunchKernelGGL(cloud_box_kernel, dim3(nchunk, bs), dim3(ICP_NT), 0, st, points, n_per_cloud, ws + L.parts,
                       (size_t)nchunk * sizeof(CloudBox), (unsigned char*)nullptr, (size_t)0, 0, N);
    int rc = check_launch("pdsc_cloud_voxel_keys");
    if (rc != PDSC_OK) return rc;
    hipLaunchKernelGGL(voxel_box_kernel, dim3(bs), dim3(ICP_NT), 0, st, (const CloudBox*)parts, box, nchunk);
    rc = check_launch("pdsc_cloud_voxel_keys");
    if (rc != PDSC_OK) return rc;
    hipLaunchKernelGGL(voxel_keys_many_kernel, dim3(nchunk, bs), dim3(ICP_NT), 0, st, points, n_per_cloud, (const CloudBox*)box, voxel,
                       keys, N);
    return check_launch("pdsc_cloud_voxel_keys");
}

int launch_cloud_voxel_means(const float* points, const double* normals, const long long* sorted_keys, const long long* perm,
                             float* out_points, double* out_normals, int* counts, int out_capacity, int renormalize, void* workspace,
                             size_t workspace_bytes, int bs, int N, int path, hipStream_t st) {
    PDSC_REQUIRE(points && normals && sorted_keys && perm && out_points && out_normals && counts && workspace,
                 "pdsc_cloud_voxel_means: null pointer");
    PDSC_REQUIRE(voxel_shape_ok(bs, N), "pdsc_cloud_voxel_means: bs=%d N=%d", bs, N);
    PDSC_REQUIRE(out_capacity >= 1 && out_capacity <= (1 << 24), "pdsc_cloud_voxel_means: out_capacity=%d outside 1 .. 2^24", out_capacity);
    PDSC_REQUIRE(renormalize == 0 || renormalize == 1, "pdsc_cloud_voxel_means: renormalize=%d is not 0 or 1", renormalize);
    PDSC_REQUIRE(path_ok(path), "pdsc_cloud_voxel_means: path=%d outside 0 .. 2", path);
    const VoxelLayout L = voxel_layout(bs, N);
    PDSC_REQUIRE(workspace_bytes >= L.bytes, "pdsc_cloud_voxel_means: workspace %zu bytes < %zu", workspace_bytes, L.bytes);
    const VoxelMeansArgs a{points, normals, sorted_keys, perm, out_points, out_normals, counts, N, out_capacity, renormalize};
    if (!path_many(path, N)) {
        hipLaunchKernelGGL(voxel_means_kernel<true>, dim3(bs), dim3(ICP_NT), 0, st, a);
        return check_launch("pdsc_cloud_voxel_means");
    }
    int* heads = reinterpret_cast<int*>((unsigned char*)workspace + L.heads);
    const int ntile = ceil_div(N, ICP_NT);
    hipLaunchKernelGGL(voxel_heads_kernel, dim3(ntile, bs), dim3(ICP_NT), 0, st, sorted_keys, heads, N);
    int rc = check_launch("pdsc_cloud_voxel_means");
    if (rc != PDSC_OK) return rc;
    hipLaunchKernelGGL(voxel_scan_kernel, dim3(bs), dim3(ICP_NT), 0, st, heads, counts, ntile, out_capacity);
    rc = check_launch("pdsc_cloud_voxel_means");
    if (rc != PDSC_OK) return rc;
    hipLaunchKernelGGL(voxel_means_many_kernel<true>, dim3(ntile, bs), dim3(ICP_NT), 0, st, a, (const int*)heads);
    return check_launch("pdsc_cloud_voxel_means");
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

extern "C" size_t pdsc_cloud_voxel_workspace_bytes(int bs, int N) { return pdsc::cloud_voxel_workspace_bytes(bs, N); }

extern "C" int pdsc_cloud_voxel_keys(const float* points, const int* n_per_cloud, double voxel_size, long long* keys, void* workspace,
                                     size_t workspace_bytes, int bs, int N, int path, void* stream) {
    return pdsc::launch_cloud_voxel_keys(points, n_per_cloud, voxel_size, keys, workspace, workspace_bytes, bs, N, path,
                                         (hipStream_t)stream);
}

extern "C" int pdsc_cloud_voxel_means(const float* points, const double* normals, const long long* sorted_keys, const long long* perm,
                                      float* out_points, double* out_normals, int* counts, int out_capacity, int renormalize,
                                      void* workspace, size_t workspace_bytes, int bs, int N, int path, void* stream) {
    return pdsc::launch_cloud_voxel_means(points, normals, sorted_keys, perm, out_points, out_normals, counts, out_capacity, renormalize,
                                          workspace, workspace_bytes, bs, N, path, (hipStream_t)stream);
}
