// f-9: the many-workgroups path of the per-cloud kernels in front of the FPFH descriptor (voxel.hip's keys and means, fpfh.hip's
// cell grid).  The one-workgroup kernels were sized for ~5 k-point clouds; on a raw scan (a quarter of a million points) one
// compute unit would work while 255 idle.  Here a cloud is cut into chunks of CLOUD_CHUNK points, one workgroup each, and every
// step is an ordinary kernel that ends before the next one starts: per-chunk partial results, then a small reduce / scan kernel,
// then the per-chunk consumer.  No kernel waits for another workgroup (no look-back flags, no cooperative launch, no grid barrier).
// What is shared here: the path selector and the per-chunk bounding box (min / max are order-free, so the reduced box is bit-equal
// to the one-workgroup one).
#pragma once
#include "icp_grid.h"

namespace pdsc {

constexpr int CLOUD_CHUNK = 1024;                   // points per workgroup (two per thread)
// path = PDSC_PATH_AUTO takes the many-workgroups kernels from this many rows on (never below 32 768, so every shape
// that ran before f-9 keeps its kernel);
// 2^30 until a raw cloud has been timed: auto never takes them, the many-workgroups path is opt-in
constexpr int CLOUD_AUTO_MANY = PDSC_CLOUD_AUTO_MANY;
static_assert(CLOUD_AUTO_MANY >= 32768, "the auto threshold stays above every pre-f-9 shape");

inline bool path_ok(int path) { return path >= PDSC_PATH_AUTO && path <= PDSC_PATH_MANY; }
inline bool path_many(int path, int N) { return path == PDSC_PATH_MANY || (path == PDSC_PATH_AUTO && N >= CLOUD_AUTO_MANY); }
__host__ __device__ inline int cloud_chunks(int N) { return (N + CLOUD_CHUNK - 1) / CLOUD_CHUNK; }

// a cloud's point count: n_per_cloud[b] clamped into 0 .. N (NULL = N each; a negative count is an empty cloud)
__device__ __forceinline__ int cloud_count(const int* __restrict__ n_per_cloud, int b, int N) {
    const int n = n_per_cloud ? n_per_cloud[b] : N;
    return n < 0 ? 0 : (n > N ? N : n);
}

struct CloudBox {                                   // 32 bytes
    float lo[3], hi[3];
    int bad, pad_;
};

// a thread's share of cloud_bounds over the reduced boxes of the chunks; returns whether a chunk met a non-finite point
__device__ __forceinline__ bool cloud_box_share(const CloudBox* __restrict__ parts, int nchunk, float (&mn)[3], float (&mx)[3]) {
    bool bad = false;
    mn[0] = mn[1] = mn[2] = INFINITY;
    mx[0] = mx[1] = mx[2] = -INFINITY;
    for (int c = threadIdx.x; c < nchunk; c += ICP_NT) {
        const CloudBox p = parts[c];
        bad |= p.bad != 0;
#pragma unroll
        for (int k = 0; k < 3; ++k) { mn[k] = fminf(mn[k], p.lo[k]); mx[k] = fmaxf(mx[k], p.hi[k]); }
    }
    return bad;
}

// grid (nchunk, bs): the box of chunk blockIdx.x of cloud blockIdx.y -> the CloudBox [nchunk] at parts_base + b parts_stride
// (bytes).  A chunk beyond the cloud's count writes the empty box.  zero_base != nullptr: the workgroups of a cloud also clear
// zero_count ints at zero_base + b zero_stride (the bucket counts of fpfh.hip's histogram kernel, which runs after the header
// kernel).
static __global__ __launch_bounds__(ICP_NT) void cloud_box_kernel(const float* __restrict__ points, const int* __restrict__ n_per_cloud,
                                                                  unsigned char* __restrict__ parts_base, size_t parts_stride,
                                                                  unsigned char* __restrict__ zero_base,
                                                                  size_t zero_stride, int zero_count, int N) {
    __shared__ float bb[ICP_NW * 6];
    const int c = blockIdx.x, nchunk = gridDim.x, b = blockIdx.y, t = threadIdx.x;
    const int n = cloud_count(n_per_cloud, b, N);
    const float* pb = points + (size_t)b * N * 3;
    const int i1 = min((c + 1) * CLOUD_CHUNK, n);
    bool bad = false;
    float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int i = c * CLOUD_CHUNK + t; i < i1; i += ICP_NT) {
        const float x = pb[(size_t)i * 3], y = pb[(size_t)i * 3 + 1], z = pb[(size_t)i * 3 + 2];
        bad |= !finite3(x, y, z);
        mn[0] = fminf(mn[0], x); mn[1] = fminf(mn[1], y); mn[2] = fminf(mn[2], z);
        mx[0] = fmaxf(mx[0], x); mx[1] = fmaxf(mx[1], y); mx[2] = fmaxf(mx[2], z);
    }
    const int any_bad = __syncthreads_or(bad);
    block_bounds(mn, mx, bb);
    if (t == 0) {
        CloudBox o;
        block_bounds_read(bb, o.lo, o.hi);
        o.bad = any_bad ? 1 : 0;
        o.pad_ = 0;
        reinterpret_cast<CloudBox*>(parts_base + (size_t)b * parts_stride)[c] = o;
    }
    if (zero_base) {
        int* z = reinterpret_cast<int*>(zero_base + (size_t)b * zero_stride);
        for (int h = c * ICP_NT + t; h < zero_count; h += nchunk * ICP_NT) z[h] = 0;
    }
}

}  // namespace pdsc
