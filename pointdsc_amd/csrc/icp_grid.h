// The nearest-target-within-a-radius search that icp.hip (f-5) and information.hip (f-6) share: one 512-thread workgroup
// counting-sorts a pair's target cloud into a hashed 3-D cell grid (cells of width >= r (1 + 1e-3)) and then looks up the 27
// neighbouring cells of each query.  The search equals brute force exactly (margin argument below); fp64 throughout.
#pragma once
#include "pdsc_common.h"

namespace pdsc {

// workgroup size of every kernel built on this header (icp.hip, information.hip, and voxel.hip, which borrows the bounds
// reduction below for clouds that are not ICP targets)
constexpr int ICP_NT = 512;
constexpr int ICP_NW = ICP_NT / 64;
// cell width = r (1 + ICP_CELL_MARGIN): a target in a cell that is not one of the 27 neighbours of the query's cell is >= r (1 + 1e-3)
// (1 - 1e-9) away along one axis, so its fp64 squared distance exceeds the fp32-rounded squared radius (relative rounding 6e-8):
// skipping it cannot change the result (the nms_grid argument of seeds.hip, in 3-D and fp64)
constexpr double ICP_CELL_MARGIN = 1e-3;
// cells per axis are capped (cell coordinates stay far inside int range; a wider cell only widens the margin)
constexpr double ICP_MAX_CELLS_PER_AXIS = 1048576.0;
// Eigen's isIdentity() at its default precision (NumTraits<double>::dummy_precision()): open3d skips transforming the source by
// an init that passes it (|T_ii - 1| <= 1e-12 min(|T_ii|, 1), |T_ij| <= 1e-12); for fp32 inits: diagonal exactly 1
constexpr double ICP_IDENTITY_PREC = 1e-12;

__host__ __device__ inline int icp_hash_size(int nt) {       // power of two >= 2 nt, >= 64
    int h = 64;
    while (h < 2 * nt) h <<= 1;
    return h;
}

// Block-wide fp64 sum of NV values per thread in a fixed order (thread-sequential, wave butterfly, waves 0..7); valid in every thread.
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
    for (int i = 0; i < NV; ++i) {
        double s = 0.0;
#pragma unroll
        for (int w = 0; w < ICP_NW; ++w) s += red[w * NV + i];
        v[i] = s;
    }
}

struct IcpGrid {
    double xmin, ymin, zmin, w;
    int nx, ny, nz, hmask;
};

__device__ __forceinline__ double icp_cell(double v, double vmin, double w) { return floor((v - vmin) / w); }

__device__ __forceinline__ int icp_bucket(int cx, int cy, int cz, int hmask) {
    return (int)(((unsigned)cx * 73856093u ^ (unsigned)cy * 19349663u ^ (unsigned)cz * 83492791u) & (unsigned)hmask);
}

// a query's cell along one axis; false when no target cell lies within one cell of it (also NaN / inf)
__device__ __forceinline__ bool icp_query_cell(double v, double vmin, double w, int n, int& ic) {
    const double c = icp_cell(v, vmin, w);
    if (!(c >= -1.0 && c <= (double)n)) return false;
    ic = (int)c;
    return true;
}

// nearest target of p with d2 < r2 (lowest original index among equal distances); returns its sorted position or -1.
// The 27 neighbour buckets' bounds are loaded first (54 independent loads in flight instead of 27 dependent round trips), then
// their targets are scanned.
__device__ __forceinline__ int icp_nearest(double px, double py, double pz, const IcpGrid& g, const float4* __restrict__ tgt,
                                           const int* __restrict__ cells, double r2, double& best_d2) {
    int qx = 0, qy = 0, qz = 0;
    const bool any = icp_query_cell(px, g.xmin, g.w, g.nx, qx) && icp_query_cell(py, g.ymin, g.w, g.ny, qy) &&
                     icp_query_cell(pz, g.zmin, g.w, g.nz, qz);
    int j0[27], j1[27];
#pragma unroll
    for (int k = 0; k < 27; ++k) {
        const int cx = qx + k % 3 - 1, cy = qy + (k / 3) % 3 - 1, cz = qz + k / 9 - 1;
        const bool ok = any && cx >= 0 && cx < g.nx && cy >= 0 && cy < g.ny && cz >= 0 && cz < g.nz;
        const int h = ok ? icp_bucket(cx, cy, cz, g.hmask) : 0;
        j0[k] = ok ? cells[h] : 0;
        j1[k] = ok ? cells[h + 1] : 0;
    }
    int best = -1, best_idx = 0x7FFFFFFF;
    best_d2 = 0.0;
#pragma unroll
    for (int k = 0; k < 27; ++k) {
        for (int j = j0[k]; j < j1[k]; ++j) {
            const float4 q = tgt[j];
            const double dx = px - (double)q.x, dy = py - (double)q.y, dz = pz - (double)q.z;
            const double d2 = dx * dx + dy * dy + dz * dz;
            const int idx = __float_as_int(q.w);
            // a bucket may be visited twice (hash collision of two neighbour cells): the minimum is idempotent
            if (d2 < r2 && (best < 0 || d2 < best_d2 || (d2 == best_d2 && idx < best_idx))) {
                best = j; best_idx = idx; best_d2 = d2;
            }
        }
    }
    return best;
}

__device__ __forceinline__ bool finite3(float x, float y, float z) { return isfinite(x) && isfinite(y) && isfinite(z); }

// Eigen isIdentity() of a row-major 4x4 at ICP_IDENTITY_PREC
__device__ __forceinline__ bool icp_is_identity(const double* T) {
    bool ident = true;
    for (int k = 0; k < 16; ++k) {
        const double v = T[k];
        if ((k % 5) == 0) ident &= fabs(v - 1.0) <= ICP_IDENTITY_PREC * fmin(fabs(v), 1.0);
        else ident &= fabs(v) <= ICP_IDENTITY_PREC;
    }
    return ident;
}

// A thread's share of a cloud's bounding box (fp32 min / max: exact; the ICP's target, voxel.hip's input cloud); returns whether
// it met a non-finite point.
__device__ __forceinline__ bool cloud_bounds(const float* __restrict__ tgtb, int nt, float (&mn)[3], float (&mx)[3]) {
    bool bad = false;
    mn[0] = mn[1] = mn[2] = INFINITY;
    mx[0] = mx[1] = mx[2] = -INFINITY;
    for (int i = threadIdx.x; i < nt; i += ICP_NT) {
        const float x = tgtb[i * 3], y = tgtb[i * 3 + 1], z = tgtb[i * 3 + 2];
        bad |= !finite3(x, y, z);
        mn[0] = fminf(mn[0], x); mn[1] = fminf(mn[1], y); mn[2] = fminf(mn[2], z);
        mx[0] = fmaxf(mx[0], x); mx[1] = fmaxf(mx[1], y); mx[2] = fmaxf(mx[2], z);
    }
    return bad;
}

// The workgroup's bounding box from the threads' shares: after the call every thread reads it from bb (ICP_NW * 6 floats of
// LDS) with block_bounds_read.
__device__ __forceinline__ void block_bounds(float (&mn)[3], float (&mx)[3], float* bb) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        for (int off = 32; off > 0; off >>= 1) {
            mn[k] = fminf(mn[k], __shfl_xor(mn[k], off, 64));
            mx[k] = fmaxf(mx[k], __shfl_xor(mx[k], off, 64));
        }
    }
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 3; ++k) { bb[wave * 6 + k] = mn[k]; bb[wave * 6 + 3 + k] = mx[k]; }
    }
    __syncthreads();
}
__device__ __forceinline__ void block_bounds_read(const float* bb, float (&lo)[3], float (&hi)[3]) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        lo[k] = bb[k]; hi[k] = bb[3 + k];
        for (int w = 1; w < ICP_NW; ++w) { lo[k] = fminf(lo[k], bb[w * 6 + k]); hi[k] = fmaxf(hi[k], bb[w * 6 + 3 + k]); }
    }
}

// The grid over the target's bounding box, written by thread 0 to *grid_s (the caller synchronises before reading it).
__device__ __forceinline__ void icp_make_grid(float (&mn)[3], float (&mx)[3], int nt, double rdist, float* bb, IcpGrid* grid_s) {
    block_bounds(mn, mx, bb);
    if (threadIdx.x == 0) {
        float lo[3], hi[3];
        block_bounds_read(bb, lo, hi);
        IcpGrid g;
        g.hmask = icp_hash_size(nt) - 1;
        if (nt > 0) {
            const double rx = (double)hi[0] - lo[0], ry = (double)hi[1] - lo[1], rz = (double)hi[2] - lo[2];
            const double rm = fmax(rx, fmax(ry, rz));
            double w = rdist * (1.0 + ICP_CELL_MARGIN);
            if (rm / w > ICP_MAX_CELLS_PER_AXIS) w = rm / ICP_MAX_CELLS_PER_AXIS;
            g.xmin = lo[0]; g.ymin = lo[1]; g.zmin = lo[2]; g.w = w;
            // the largest target coordinate lands in cell floor(range / w) by the same expression as icp_cell
            g.nx = (int)floor(rx / w) + 1; g.ny = (int)floor(ry / w) + 1; g.nz = (int)floor(rz / w) + 1;
        } else {
            g.xmin = g.ymin = g.zmin = 0.0; g.w = 1.0;
            g.nx = g.ny = g.nz = 0;                                    // no cells: every query finds nothing
        }
        *grid_s = g;
    }
}

// the bucket of a target point (its cell is clamped into the grid: never taken, the same expression as nx; kept as a guard)
__device__ __forceinline__ int icp_target_bucket(float x, float y, float z, const IcpGrid& g) {
    int cx = (int)icp_cell(x, g.xmin, g.w), cy = (int)icp_cell(y, g.ymin, g.w), cz = (int)icp_cell(z, g.zmin, g.w);
    cx = cx < 0 ? 0 : (cx >= g.nx ? g.nx - 1 : cx);
    cy = cy < 0 ? 0 : (cy >= g.ny ? g.ny - 1 : cy);
    cz = cz < 0 ? 0 : (cz >= g.nz ? g.nz - 1 : cz);
    return icp_bucket(cx, cy, cz, g.hmask);
}

// One workgroup: bucket counts cells[0, hsize) -> their exclusive scan in cells and cursor, cells[hsize] = the total: `per`
// consecutive buckets per thread, Hillis-Steele over the thread totals.  scan: ICP_NT ints of LDS.
__device__ __forceinline__ void icp_scan_cells(int* cells, int* cursor, int hsize, int* scan) {
    const int t = threadIdx.x;
    const int per = (hsize + ICP_NT - 1) / ICP_NT;
    const int h0 = t * per, h1 = min(h0 + per, hsize);
    int local = 0;
    for (int h = h0; h < h1; ++h) local += cells[h];
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
        const int c = cells[h];
        cells[h] = run;
        cursor[h] = run;
        run += c;
    }
    if (t == ICP_NT - 1) cells[hsize] = scan[t];                       // == nt
}

// Counting sort of the target into the grid's hsize = hmask + 1 buckets: cells[h] .. cells[h + 1] bound bucket h in tsort
// (float4 {x, y, z, original index}).  cells: hsize + 1 ints, cursor: hsize ints (global), scan: ICP_NT ints of LDS.  The caller
// synchronises before the first search.
__device__ __forceinline__ void icp_sort_target(const float* __restrict__ tgtb, int nt, const IcpGrid& g, int* cells, int* cursor,
                                                float4* tsort, int* scan) {
    const int t = threadIdx.x;
    const int hsize = g.hmask + 1;
    for (int h = t; h <= hsize; h += ICP_NT) cells[h] = 0;
    __syncthreads();
    for (int i = t; i < nt; i += ICP_NT) atomicAdd(&cells[icp_target_bucket(tgtb[i * 3], tgtb[i * 3 + 1], tgtb[i * 3 + 2], g)], 1);
    __syncthreads();
    icp_scan_cells(cells, cursor, hsize, scan);
    __syncthreads();
    for (int i = t; i < nt; i += ICP_NT) {
        const float x = tgtb[i * 3], y = tgtb[i * 3 + 1], z = tgtb[i * 3 + 2];
        const int pos = atomicAdd(&cursor[icp_target_bucket(x, y, z, g)], 1);
        tsort[pos] = make_float4(x, y, z, __int_as_float(i));          // order inside a bucket is free: the search is order-independent
    }
}

}  // namespace pdsc
