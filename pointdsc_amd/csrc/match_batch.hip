// f-19: correspondence construction for a batch of pairs over a pool of clouds -- the batched form of match.hip (f-2).
//   reference: datasets/ThreeDMatch.py:283-308 / datasets/KITTI.py:80-105 inside Dataset.__getitem__, once per pair:
//     distance, argmin (+ mutual check), the ground-truth label, the keypoint gather, corr_pos = concat - column mean.
// The pool's descriptors and keypoints arrive concatenated; an int32 table on the device lists the work items
//     table[w] = { source offset, source count, target offset, target count, first source tile }        (rows of the pool, 5 ints)
// one per pair, or two per pair with the mutual check (item 2p: source -> target, item 2p + 1: target -> source).
// Four launches after the key fill, whatever the number of pairs:
//   match_nn_ragged_kernel   grid (source tiles of ALL items, target splits); a workgroup finds its item by bisection of the
//                            first-tile column and runs match_tile (match_tile.h: the single-pair kernel's body, same bits)
//   corr_select_batch_kernel one workgroup per pair: corr, num_corr, zero rows behind the count
//   corr_gather_batch_kernel (1024-row chunks, pairs): gather, fp64 label, fp64 column sums per chunk, zero rows behind the count
//   corr_centre_batch_kernel (1024-row chunks, pairs): the chunks' sums added in ascending chunk order, corr_pos = concat - mean
#include "match_tile.h"

namespace pdsc {

constexpr int CB_COLS = 5;            // ints per work item
constexpr int CB_ROWS = 1024;         // rows of a pair per gather / centre workgroup

template <int MODE>
__global__ __launch_bounds__(256) void match_nn_ragged_kernel(const float* __restrict__ desc, const int* __restrict__ table, int W, int D,
                                                              int tgt_per_split, unsigned long long* __restrict__ keys) {
    // the last item whose first tile is <= this tile (first tiles ascend strictly: every item has at least one row)
    int lo = 0, hi = W - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (table[CB_COLS * mid + 4] <= (int)blockIdx.x) lo = mid;
        else hi = mid - 1;
    }
    const int* e = table + CB_COLS * lo;
    const int src_off = e[0], ns = e[1], tgt_off = e[2], nt = e[3], tile0 = e[4];
    const int j_begin = blockIdx.y * tgt_per_split;
    if (j_begin >= nt) return;                                       // a short target cloud: nothing in this split (uniform)
    match_tile<MODE>(desc + (size_t)src_off * D, desc + (size_t)tgt_off * D, ns, D, ((int)blockIdx.x - tile0) * MT_SRC, j_begin,
                     min(nt, j_begin + tgt_per_split), keys + (size_t)tile0 * MT_SRC);
}

// corr[p][c] = (i, s2t[i]) for the kept i in ascending order, num_corr[p] = rows kept, rows behind them zero.  The indices are the
// low words of the matcher's keys (item w at keys + first_tile[w] * MT_SRC).  One workgroup per pair, scan in chunks of 1024.
__global__ __launch_bounds__(1024) void corr_select_batch_kernel(const unsigned long long* __restrict__ keys, const int* __restrict__ table,
                                                                 int mutual, int cap, int* __restrict__ corr, int* __restrict__ num_corr) {
    __shared__ int wave_tot[16];
    __shared__ int base;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int p = blockIdx.x, w = mutual ? 2 * p : p;
    const int Ns = table[CB_COLS * w + 1], Nt = table[CB_COLS * w + 3];
    const unsigned long long* s2t = keys + (size_t)table[CB_COLS * w + 4] * MT_SRC;
    const unsigned long long* t2s = mutual ? keys + (size_t)table[CB_COLS * (w + 1) + 4] * MT_SRC : nullptr;
    int* out = corr + (size_t)p * cap * 2;
    if (t == 0) base = 0;
    __syncthreads();
    for (int i0 = 0; i0 < Ns; i0 += 1024) {
        const int i = i0 + t;
        int keep = 0, j = 0;
        if (i < Ns) {
            j = (int)(unsigned int)(s2t[i] & 0xffffffffu);
            keep = (unsigned int)j < (unsigned int)Nt;                // always: every row met target 0 (the guard keeps the read below in range)
            if (keep && mutual) keep = (int)(unsigned int)(t2s[j] & 0xffffffffu) == i;
        }
        int incl = keep;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int up = __shfl_up(incl, off, 64);
            if (lane >= off) incl += up;
        }
        if (lane == 63) wave_tot[wave] = incl;
        __syncthreads();
        int offs = base;
        for (int k = 0; k < wave; ++k) offs += wave_tot[k];
        if (keep) {
            const int c = offs + incl - 1;
            if (c < cap) {                                           // cap >= Ns is the caller's promise; a short one loses rows, never memory
                out[2 * c] = i;
                out[2 * c + 1] = j;
            }
        }
        __syncthreads();
        if (t == 1023) base = offs + incl;
        __syncthreads();
    }
    const int n = min(base, cap);
    for (int c = n + t; c < cap; c += 1024) {
        out[2 * c] = 0;
        out[2 * c + 1] = 0;
    }
    if (t == 0) num_corr[p] = n;
}

// rows [1024 chunk, +1024) of pair p: src_sel / tgt_sel, the label, the chunk's fp64 column sums -> partial[p][chunk][6];
// rows from num_corr[p] up to cap are written as zeros in every output.
//   label (datasets/ThreeDMatch.py:293-297, fp64 as numpy promotes it): sqrt(sum((R x + t - y)^2)) < thr
__global__ __launch_bounds__(1024) void corr_gather_batch_kernel(const float* __restrict__ keypts, const int* __restrict__ table,
                                                                 const int* __restrict__ corr, const int* __restrict__ num_corr, int mutual,
                                                                 int cap, const double* __restrict__ gt_trans, double thr,
                                                                 float* __restrict__ corr_pos, float* __restrict__ src_sel,
                                                                 float* __restrict__ tgt_sel, float* __restrict__ labels,
                                                                 double* __restrict__ partial) {
    __shared__ double red[16][6];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int p = blockIdx.y, w = mutual ? 2 * p : p;
    const int n = num_corr[p];
    const float* src_kp = keypts + (size_t)table[CB_COLS * w] * 3;
    const float* tgt_kp = keypts + (size_t)table[CB_COLS * w + 2] * 3;
    const int c = blockIdx.x * CB_ROWS + t;
    const size_t row = (size_t)p * cap + c;
    double s[6] = {0, 0, 0, 0, 0, 0};
    if (c < n) {
        const int i = corr[2 * row], j = corr[2 * row + 1];
        float a[3], b[3];
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            a[d] = src_kp[(size_t)i * 3 + d];
            b[d] = tgt_kp[(size_t)j * 3 + d];
            src_sel[row * 3 + d] = a[d];
            tgt_sel[row * 3 + d] = b[d];
            s[d] = (double)a[d];
            s[3 + d] = (double)b[d];
        }
        if (labels) {
            const double* T = gt_trans + (size_t)p * 16;
            double sq = 0.0;
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                const double warped = ((T[4 * d] * (double)a[0] + T[4 * d + 1] * (double)a[1]) + T[4 * d + 2] * (double)a[2]) + T[4 * d + 3];
                const double diff = warped - (double)b[d];
                sq += diff * diff;
            }
            labels[row] = sqrt(sq) < thr ? 1.f : 0.f;
        }
    } else if (c < cap) {
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            src_sel[row * 3 + d] = 0.f;
            tgt_sel[row * 3 + d] = 0.f;
            corr_pos[row * 6 + d] = 0.f;
            corr_pos[row * 6 + 3 + d] = 0.f;
        }
        if (labels) labels[row] = 0.f;
    }
#pragma unroll
    for (int d = 0; d < 6; ++d) s[d] = wave_sum(s[d]);
    if (lane == 0) {
#pragma unroll
        for (int d = 0; d < 6; ++d) red[wave][d] = s[d];
    }
    __syncthreads();
    if (t < 6) {
        double tot = 0;
        for (int k = 0; k < 16; ++k) tot += red[k][t];
        partial[((size_t)p * gridDim.x + blockIdx.x) * 6 + t] = tot;
    }
}

// corr_pos = concat(src_sel, tgt_sel) - column mean over the pair's num_corr rows; the chunk sums are added in ascending chunk order
// by every workgroup of the pair alike (fixed order: the mean does not depend on scheduling)
__global__ __launch_bounds__(1024) void corr_centre_batch_kernel(const int* __restrict__ num_corr, int cap, const float* __restrict__ src_sel,
                                                                 const float* __restrict__ tgt_sel, const double* __restrict__ partial,
                                                                 float* __restrict__ corr_pos) {
    __shared__ float mean[6];
    const int t = threadIdx.x, p = blockIdx.y;
    const int n = num_corr[p];
    if ((int)blockIdx.x * CB_ROWS >= n) return;                      // uniform: only zero rows here, written by the gather
    if (t < 6) {
        double tot = 0;
        for (int k = 0; k < (int)gridDim.x; ++k) tot += partial[((size_t)p * gridDim.x + k) * 6 + t];
        mean[t] = (float)(tot / (double)n);
    }
    __syncthreads();
    const int c = blockIdx.x * CB_ROWS + t;
    if (c < n) {
        const size_t row = (size_t)p * cap + c;
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            corr_pos[row * 6 + d] = src_sel[row * 3 + d] - mean[d];
            corr_pos[row * 6 + 3 + d] = tgt_sel[row * 3 + d] - mean[3 + d];
        }
    }
}

}  // namespace pdsc

using namespace pdsc;

static size_t cb_keys_bytes(int total_tiles) { return (size_t)total_tiles * MT_SRC * sizeof(unsigned long long); }

extern "C" size_t pdsc_corr_batch_workspace_bytes(int P, int total_tiles, int cap) {
    if (P <= 0 || total_tiles <= 0 || cap <= 0) return 0;
    return cb_keys_bytes(total_tiles) + (size_t)P * ceil_div(cap, CB_ROWS) * 6 * sizeof(double);
}

extern "C" int pdsc_build_correspondences_batch_ex(const float* desc, const float* keypts, const int* table, int P, int D, int mutual,
                                                   int metric, int total_tiles, int max_tgt, int cap, const double* gt_trans,
                                                   double inlier_threshold, float* corr_pos, float* src_sel, float* tgt_sel, int* corr,
                                                   int* num_corr, float* gt_labels, void* workspace, size_t workspace_bytes, int splits,
                                                   void* stream) {
    PDSC_REQUIRE(desc && keypts && table && corr_pos && src_sel && tgt_sel && corr && num_corr && workspace,
                 "pdsc_build_correspondences_batch: null pointer");
    PDSC_REQUIRE(P >= 1 && P <= 65535 && D >= 1 && D <= MT_MAXD, "pdsc_build_correspondences_batch: P=%d D=%d (1 <= P <= 65535, 1 <= D <= %d)",
                 P, D, MT_MAXD);
    PDSC_REQUIRE((mutual == 0 || mutual == 1) && (metric == 0 || metric == 1),
                 "pdsc_build_correspondences_batch: mutual=%d metric=%d (each 0 or 1)", mutual, metric);
    const long long W = (long long)P * (mutual ? 2 : 1);
    PDSC_REQUIRE(total_tiles >= W && max_tgt >= 1 && max_tgt <= 65535 * MT_TGT && cap >= 1,
                 "pdsc_build_correspondences_batch: total_tiles=%d (>= %lld work items) max_tgt=%d cap=%d", total_tiles, W, max_tgt, cap);
    PDSC_REQUIRE((gt_trans != nullptr) == (gt_labels != nullptr), "pdsc_build_correspondences_batch: gt_trans and gt_labels go together");
    PDSC_REQUIRE(!gt_trans || inlier_threshold == inlier_threshold, "pdsc_build_correspondences_batch: inlier_threshold is NaN");
    const int max_splits = ceil_div(max_tgt, MT_TGT);
    PDSC_REQUIRE(splits >= 0 && splits <= max_splits, "pdsc_build_correspondences_batch: splits=%d (0 = the fill rule, or 1 .. %d)", splits,
                 max_splits);
    const size_t need = pdsc_corr_batch_workspace_bytes(P, total_tiles, cap);
    if (workspace_bytes < need) {
        set_error("pdsc_build_correspondences_batch: workspace %zu < %zu bytes", workspace_bytes, need);
        return PDSC_ERR_WORKSPACE;
    }
    hipStream_t st = (hipStream_t)stream;
    unsigned long long* keys = (unsigned long long*)workspace;
    double* partial = (double*)((char*)workspace + cb_keys_bytes(total_tiles));
    if (const int rc = launch_fill_u32((unsigned int*)keys, 0xFFFFFFFFu, (size_t)total_tiles * MT_SRC * 2, st); rc != PDSC_OK) return rc;
    // match_launch's rule on the batch's tile total: a large batch runs with one split, no merge traffic beyond one key per row
    int nsplit;
    const int per = match_split_plan(total_tiles, max_tgt, splits, &nsplit);
    if (metric == 0) hipLaunchKernelGGL(match_nn_ragged_kernel<0>, dim3(total_tiles, nsplit), dim3(256), 0, st, desc, table, (int)W, D, per, keys);
    else hipLaunchKernelGGL(match_nn_ragged_kernel<1>, dim3(total_tiles, nsplit), dim3(256), 0, st, desc, table, (int)W, D, per, keys);
    int rc = check_launch("pdsc_build_correspondences_batch(match)");
    if (rc != PDSC_OK) return rc;
    hipLaunchKernelGGL(corr_select_batch_kernel, dim3(P), dim3(1024), 0, st, keys, table, mutual, cap, corr, num_corr);
    rc = check_launch("pdsc_build_correspondences_batch(select)");
    if (rc != PDSC_OK) return rc;
    const dim3 grid(ceil_div(cap, CB_ROWS), P);
    hipLaunchKernelGGL(corr_gather_batch_kernel, grid, dim3(1024), 0, st, keypts, table, corr, num_corr, mutual, cap, gt_trans,
                       inlier_threshold, corr_pos, src_sel, tgt_sel, gt_labels, partial);
    rc = check_launch("pdsc_build_correspondences_batch(gather)");
    if (rc != PDSC_OK) return rc;
    hipLaunchKernelGGL(corr_centre_batch_kernel, grid, dim3(1024), 0, st, num_corr, cap, src_sel, tgt_sel, partial, corr_pos);
    return check_launch("pdsc_build_correspondences_batch(centre)");
}

extern "C" int pdsc_build_correspondences_batch(const float* desc, const float* keypts, const int* table, int P, int D, int mutual,
                                                int metric, int total_tiles, int max_tgt, int cap, const double* gt_trans,
                                                double inlier_threshold, float* corr_pos, float* src_sel, float* tgt_sel, int* corr,
                                                int* num_corr, float* gt_labels, void* workspace, size_t workspace_bytes, void* stream) {
    return pdsc_build_correspondences_batch_ex(desc, keypts, table, P, D, mutual, metric, total_tiles, max_tgt, cap, gt_trans,
                                               inlier_threshold, corr_pos, src_sel, tgt_sel, corr, num_corr, gt_labels, workspace,
                                               workspace_bytes, 0, stream);
}
