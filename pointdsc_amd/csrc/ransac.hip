// f-21: correspondence RANSAC (baseline_scripts/baseline_3DMatch.py:80-98 --method RANSAC; evaluation/test_3DMatch.py:59-77 and
// test_KITTI.py:59-77 --solver RANSAC), modelled on open3d 0.9 RegistrationRANSACBasedOnCorrespondence.  The contract and its named
// rules (DRAW_RULE, SCORE_RULE, SELECT_RULE, NO_REFIT_RULE) are written out in include/pointdsc_hip.h and DESIGN.md section 8 f-21.
// Four launches per call, fp64 throughout:
//   compact      mask -> the ascending candidate list L and its length M per pair (block scan of wave ballots: no atomics, no reorder)
//   hypothesise  one lane per hypothesis: draw (or read) the sample, Eigen's umeyama without scaling through kabsch_from_covariance_f64,
//                the 12 pose values to the hypothesis table
//   score        the hot path: one lane per hypothesis with its pose in registers; the workgroup stages RANSAC_CHUNK consecutive entries
//                of L into LDS as widened src / tgt rows, every lane walks them in list order (all lanes of a wave read the same LDS
//                address: a broadcast) and keeps its own count and sum of squares -- no cross-lane reduction, no atomics
//   select       one workgroup per pair: the chunk partials of a split launch added in ascending order, SELECT_RULE, labels and outputs
// The solve is a launch of its own and not the prologue of the scoring lanes: it runs once per hypothesis, not once per point chunk
// of a split launch, and its registers (the Jacobi body) do not set the scoring kernel's occupancy.
// DETERMINISM: a hypothesis's sumsq is DEFINED as ((p_0 + p_1) + p_2) + ... over the partial sums p_c of the fixed chunks
// [c RANSAC_CHUNK, (c + 1) RANSAC_CHUNK) of L, each chunk summed in list order.  A launch that gives every chunk its own workgroup
// (small batches: one pair of 5000 hypotheses is 79 wavefronts) and a launch whose workgroups walk all chunks compute exactly that,
// so a pair's bits depend neither on the batch nor on the tiling; chunks past M add +0.0.  Bound: fp64 vector rate (reported in
// DESIGN.md as achieved operations per second against I M RANSAC_OPS_PER_POINT).
#include "pdsc_common.h"

namespace pdsc {
namespace {

constexpr int RANSAC_NT = 256;                       // lanes (hypotheses) per workgroup of the hypothesise and score kernels
constexpr int RANSAC_CHUNK = PDSC_RANSAC_CHUNK;      // entries of L per staged chunk: 512 x 48 bytes = 24 KiB of LDS
constexpr int RANSAC_SEL_NT = 1024;                  // compact / select: one workgroup per pair
constexpr int RANSAC_SPLIT_BELOW = 1024;             // fewer hypothesis workgroups than this in a launch: one workgroup per chunk

struct RansacLayout {
    size_t list, m, pose, count, sumsq, pcount, psumsq, total;
    int nchunk, split;
};

inline RansacLayout ransac_layout(int bs, int N, int I) {
    RansacLayout L;
    L.nchunk = ceil_div(N, RANSAC_CHUNK);
    const long long tiles = ceil_div(I, RANSAC_NT);
    L.split = (L.nchunk > 1 && (long long)bs * tiles < RANSAC_SPLIT_BELOW) ? 1 : 0;
    const long long H = (long long)bs * I;
    size_t o = 0;
    L.list = o;   o += (size_t)round_up((long long)bs * N * 4, 256);
    L.m = o;      o += (size_t)round_up((long long)bs * 4, 256);
    L.pose = o;   o += (size_t)round_up(H * 96, 256);                      // used when the caller does not take the table
    L.count = o;  o += (size_t)round_up(H * 4, 256);
    L.sumsq = o;  o += (size_t)round_up(H * 8, 256);
    L.pcount = o; o += L.split ? (size_t)round_up(H * L.nchunk * 4, 256) : 0;
    L.psumsq = o; o += L.split ? (size_t)round_up(H * L.nchunk * 8, 256) : 0;
    L.total = o;
    return L;
}

// DRAW_RULE: splitmix64's output for the state seed + (c + 1) * golden gamma
__device__ __forceinline__ unsigned long long ransac_splitmix(unsigned long long seed, unsigned long long c) {
    unsigned long long z = seed + (c + 1ull) * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// SCORE_RULE: d2 = |R p + t - q|^2 in fp64.  The scoring pass and the label pass both call this one function, so the labels of the
// winner are exactly the points its count counted.
__device__ __forceinline__ double ransac_d2(const double (&T)[12], double x, double y, double z, double qx, double qy, double qz) {
    const double dx = fma(T[2], z, fma(T[1], y, fma(T[0], x, T[3]))) - qx;
    const double dy = fma(T[6], z, fma(T[5], y, fma(T[4], x, T[7]))) - qy;
    const double dz = fma(T[10], z, fma(T[9], y, fma(T[8], x, T[11]))) - qz;
    return fma(dz, dz, fma(dy, dy, dx * dx));
}

// ---- compaction: L = ascending indices with mask > 0 among the pair's first n_b rows (no mask: 0 .. n_b - 1), M = |L| ----
__global__ __launch_bounds__(RANSAC_SEL_NT) void ransac_compact_kernel(const float* __restrict__ mask, const int* __restrict__ counts,
                                                                       int* __restrict__ list, int* __restrict__ Mout, int N) {
    __shared__ int wave_tot[RANSAC_SEL_NT / PDSC_WAVE];
    __shared__ int base_s;
    const int b = blockIdx.x, t = threadIdx.x, lane = t & (PDSC_WAVE - 1), w = t / PDSC_WAVE;
    int nb = counts ? counts[b] : N;
    nb = nb < 0 ? 0 : (nb > N ? N : nb);
    int* Lb = list + (size_t)b * N;
    if (!mask) {
        for (int i = t; i < nb; i += RANSAC_SEL_NT) Lb[i] = i;
        if (t == 0) Mout[b] = nb;
        return;
    }
    const float* mb = mask + (size_t)b * N;
    if (t == 0) base_s = 0;
    __syncthreads();
    for (int i0 = 0; i0 < nb; i0 += RANSAC_SEL_NT) {
        const int i = i0 + t;
        const bool in = i < nb && mb[i] > 0.0f;
        const unsigned long long bal = __ballot(in);
        const int before = __popcll(bal & ((1ull << lane) - 1ull));
        if (lane == 0) wave_tot[w] = __popcll(bal);
        __syncthreads();
        int off = base_s;
        for (int k = 0; k < w; ++k) off += wave_tot[k];
        if (in) Lb[off + before] = i;
        __syncthreads();
        if (t == 0) {
            int tot = 0;
            for (int k = 0; k < RANSAC_SEL_NT / PDSC_WAVE; ++k) tot += wave_tot[k];
            base_s += tot;
        }
        __syncthreads();
    }
    if (t == 0) Mout[b] = base_s;
}

// ---- hypotheses: one lane draws (or reads) its sample and solves it ----
__global__ __launch_bounds__(RANSAC_NT) void ransac_hypothesis_kernel(const float* __restrict__ src, const float* __restrict__ tgt,
                                                                      const int* __restrict__ list, const int* __restrict__ Mv,
                                                                      const int* __restrict__ samples, int enabled, int n, int I,
                                                                      unsigned long long seed, long long pair_offset,
                                                                      double* __restrict__ pose, int N) {
    const int b = blockIdx.y;
    const int i = blockIdx.x * RANSAC_NT + threadIdx.x;
    if (i >= I) return;
    const int M = Mv[b];
    const int* Lb = list + (size_t)b * N;
    const float* sb = src + (size_t)b * N * 3;
    const float* tb = tgt + (size_t)b * N * 3;
    const size_t h = (size_t)b * I + i;
    const unsigned long long c0 = (((unsigned long long)(pair_offset + b)) * (unsigned long long)I + (unsigned long long)i) * 8ull;
    bool valid = enabled && M >= n;                                           // the early outs: nothing wins
    auto position = [&](int j) -> int {
        if (samples) return samples[h * n + j];
        return (int)(((ransac_splitmix(seed, c0 + j) >> 32) * (unsigned long long)M) >> 32);
    };
    double T[16];
    if (valid) {
        // the sample is gathered twice (sums, then the demeaned covariance) and not held: ransac_n is a run-time value, and a
        // local array indexed by it would live in scratch memory
        double sa[3] = {0, 0, 0}, sq[3] = {0, 0, 0};
        for (int j = 0; j < n; ++j) {
            const int pos = position(j);
            if (pos < 0 || pos >= M) { valid = false; break; }
            const int idx = Lb[pos];
#pragma unroll
            for (int k = 0; k < 3; ++k) { sa[k] += (double)sb[idx * 3 + k]; sq[k] += (double)tb[idx * 3 + k]; }
        }
        if (valid) {
            const double one_over_n = 1.0 / (double)n;
            const double mA[3] = {sa[0] * one_over_n, sa[1] * one_over_n, sa[2] * one_over_n};
            const double mB[3] = {sq[0] * one_over_n, sq[1] * one_over_n, sq[2] * one_over_n};
            double H[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
            for (int j = 0; j < n; ++j) {
                const int idx = Lb[position(j)];
                const double a[3] = {(double)sb[idx * 3] - mA[0], (double)sb[idx * 3 + 1] - mA[1], (double)sb[idx * 3 + 2] - mA[2]};
                const double q[3] = {(double)tb[idx * 3] - mB[0], (double)tb[idx * 3 + 1] - mB[1], (double)tb[idx * 3 + 2] - mB[2]};
#pragma unroll
                for (int r = 0; r < 3; ++r)
#pragma unroll
                    for (int c = 0; c < 3; ++c) H[r * 3 + c] += a[r] * q[c];
            }
#pragma unroll
            for (int k = 0; k < 9; ++k) H[k] *= one_over_n;
            kabsch_from_covariance_f64(H, mA, mB, T);
#pragma unroll
            for (int k = 0; k < 12; ++k) valid = valid && isfinite(T[k]);
        }
    }
    double* out = pose + h * 12;
#pragma unroll
    for (int k = 0; k < 12; ++k) out[k] = valid ? T[k] : __builtin_nan("");
}

// ---- scoring: count and sum of squares of every hypothesis over every candidate ----
__global__ __launch_bounds__(RANSAC_NT) void ransac_score_kernel(const float* __restrict__ src, const float* __restrict__ tgt,
                                                                 const int* __restrict__ list, const int* __restrict__ Mv,
                                                                 const double* __restrict__ pose, double r2, int* __restrict__ hyp_count,
                                                                 double* __restrict__ hyp_sumsq, int* __restrict__ pcount,
                                                                 double* __restrict__ psumsq, int I, int N, int nchunk, int split) {
    __shared__ double pts[RANSAC_CHUNK * 6];
    const int b = blockIdx.z, t = threadIdx.x;
    const int i = blockIdx.x * RANSAC_NT + t;
    const int M = Mv[b];
    const int* Lb = list + (size_t)b * N;
    const float* sb = src + (size_t)b * N * 3;
    const float* tb = tgt + (size_t)b * N * 3;
    const size_t h = (size_t)b * I + (i < I ? i : 0);
    double T[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) T[k] = pose[h * 12 + k];          // an invalid hypothesis: NaN, every comparison below is false
    const int c_begin = split ? (int)blockIdx.y : 0;
    const int c_end = split ? c_begin + 1 : nchunk;
    int total_count = 0;
    double total_sumsq = 0.0;
    for (int c = c_begin; c < c_end; ++c) {
        const int base = c * RANSAC_CHUNK;
        int len = M - base;
        len = len > RANSAC_CHUNK ? RANSAC_CHUNK : len;             // the same for the whole workgroup
        int count = 0;
        double sumsq = 0.0;
        if (len > 0) {
            __syncthreads();                                       // the previous chunk has been read
            for (int e = t; e < len; e += RANSAC_NT) {
                const int idx = Lb[base + e];
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    pts[e * 6 + k] = (double)sb[idx * 3 + k];
                    pts[e * 6 + 3 + k] = (double)tb[idx * 3 + k];
                }
            }
            __syncthreads();
#pragma unroll 4
            for (int e = 0; e < len; ++e) {
                const double* p = pts + e * 6;
                const double d2 = ransac_d2(T, p[0], p[1], p[2], p[3], p[4], p[5]);
                const bool in = d2 < r2;
                count += in ? 1 : 0;
                sumsq += in ? d2 : 0.0;
            }
        }
        if (split) {
            if (i < I) {
                const size_t o = ((size_t)b * nchunk + c) * I + i;
                pcount[o] = count;
                psumsq[o] = sumsq;
            }
        } else {
            total_count += count;
            total_sumsq += sumsq;                                  // ascending chunks: the sum's definition
        }
    }
    if (!split && i < I) {
        hyp_count[h] = total_count;
        hyp_sumsq[h] = total_sumsq;
    }
}

struct RansacBest {
    int count;
    double sumsq;
    int iter;
};
// SELECT_RULE as a total order: larger count, then smaller sumsq, then lower iteration
__device__ __forceinline__ bool ransac_better(const RansacBest& a, const RansacBest& b) {
    if (a.count != b.count) return a.count > b.count;
    if (a.sumsq != b.sumsq) return a.sumsq < b.sumsq;
    return a.iter < b.iter;
}

// ---- selection and outputs: one workgroup per pair ----
__global__ __launch_bounds__(RANSAC_SEL_NT) void ransac_select_kernel(const float* __restrict__ src, const float* __restrict__ tgt,
                                                                      const int* __restrict__ list, const int* __restrict__ Mv,
                                                                      const double* __restrict__ pose, double r2, int* __restrict__ hyp_count,
                                                                      double* __restrict__ hyp_sumsq, const int* __restrict__ pcount,
                                                                      const double* __restrict__ psumsq, float* __restrict__ trans,
                                                                      float* __restrict__ labels, double* __restrict__ fitness,
                                                                      double* __restrict__ rmse, int* __restrict__ best_iter,
                                                                      int* __restrict__ num_candidates, int I, int N, int nchunk, int split) {
    __shared__ int red_count[RANSAC_SEL_NT];
    __shared__ double red_sumsq[RANSAC_SEL_NT];
    __shared__ int red_iter[RANSAC_SEL_NT];
    __shared__ double Tw[12];
    const int b = blockIdx.x, t = threadIdx.x;
    const int M = Mv[b];
    const size_t hb = (size_t)b * I;
    RansacBest best = {0, 0.0, I};                                 // count 0 never wins
    for (int i = t; i < I; i += RANSAC_SEL_NT) {
        int count;
        double sumsq;
        if (split) {
            count = 0;
            sumsq = 0.0;
            for (int c = 0; c < nchunk; ++c) {                     // ascending chunks, one owner: the sum's definition
                const size_t o = ((size_t)b * nchunk + c) * I + i;
                count += pcount[o];
                sumsq += psumsq[o];
            }
            hyp_count[hb + i] = count;
            hyp_sumsq[hb + i] = sumsq;
        } else {
            count = hyp_count[hb + i];
            sumsq = hyp_sumsq[hb + i];
        }
        const RansacBest cand = {count, sumsq, i};
        if (count > 0 && ransac_better(cand, best)) best = cand;
    }
    red_count[t] = best.count; red_sumsq[t] = best.sumsq; red_iter[t] = best.iter;
    __syncthreads();
    for (int s = RANSAC_SEL_NT / 2; s > 0; s >>= 1) {
        if (t < s) {
            const RansacBest a = {red_count[t], red_sumsq[t], red_iter[t]};
            const RansacBest o = {red_count[t + s], red_sumsq[t + s], red_iter[t + s]};
            if (ransac_better(o, a)) { red_count[t] = o.count; red_sumsq[t] = o.sumsq; red_iter[t] = o.iter; }
        }
        __syncthreads();
    }
    const int win_count = red_count[0];
    const double win_sumsq = red_sumsq[0];
    const int win = win_count > 0 ? red_iter[0] : -1;
    if (t < 12) Tw[t] = win >= 0 ? pose[(hb + win) * 12 + t] : ((t % 5) == 0 ? 1.0 : 0.0);
    float* lb = labels + (size_t)b * N;
    for (int i = t; i < N; i += RANSAC_SEL_NT) lb[i] = 0.0f;
    __syncthreads();                                               // the zeros are written, Tw is visible
    if (t < 16) trans[(size_t)b * 16 + t] = t < 12 ? (float)Tw[t] : (t == 15 ? 1.0f : 0.0f);
    if (t == 0) {
        fitness[b] = win >= 0 ? (double)win_count / (double)M : 0.0;
        rmse[b] = win >= 0 ? sqrt(win_sumsq / (double)win_count) : 0.0;
        best_iter[b] = win;
        num_candidates[b] = M;
    }
    if (win < 0) return;
    double T[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) T[k] = Tw[k];
    const int* Lb = list + (size_t)b * N;
    const float* sb = src + (size_t)b * N * 3;
    const float* tb = tgt + (size_t)b * N * 3;
    for (int e = t; e < M; e += RANSAC_SEL_NT) {
        const int idx = Lb[e];
        const double d2 = ransac_d2(T, (double)sb[idx * 3], (double)sb[idx * 3 + 1], (double)sb[idx * 3 + 2], (double)tb[idx * 3],
                                    (double)tb[idx * 3 + 1], (double)tb[idx * 3 + 2]);
        if (d2 < r2) lb[idx] = 1.0f;
    }
}

inline bool ransac_sizes_ok(int bs, int N, int I) {
    return bs >= 1 && bs <= PDSC_RANSAC_MAX_PAIRS && N >= 1 && N <= PDSC_RANSAC_MAX_N && I >= 1 && I <= PDSC_RANSAC_MAX_ITERATIONS;
}

}  // namespace

size_t ransac_workspace_bytes(int bs, int N, int I) { return ransac_sizes_ok(bs, N, I) ? ransac_layout(bs, N, I).total : 0; }

int launch_ransac_correspondence(const float* src, const float* tgt, const int* counts, const float* mask, const int* samples, double r,
                                 int ransac_n, int I, unsigned long long seed, long long pair_offset, float* trans, float* labels,
                                 double* fitness, double* inlier_rmse, int* best_iter, int* num_candidates, double* hyp_trans,
                                 int* hyp_count, double* hyp_sumsq, void* workspace, size_t workspace_bytes, int bs, int N,
                                 hipStream_t st, float* stage_ms) {
    PDSC_REQUIRE(src && tgt && trans && labels && fitness && inlier_rmse && best_iter && num_candidates && workspace,
                 "pdsc_ransac_correspondence: null pointer");
    PDSC_REQUIRE(ransac_n >= 3 && ransac_n <= 8, "pdsc_ransac_correspondence: ransac_n=%d outside 3..8", ransac_n);
    PDSC_REQUIRE(I >= 1, "pdsc_ransac_correspondence: max_iteration=%d < 1", I);
    PDSC_REQUIRE(ransac_sizes_ok(bs, N, I), "pdsc_ransac_correspondence: bs=%d N=%d I=%d outside 1..%d, 1..%d, 1..%d", bs, N, I,
                 PDSC_RANSAC_MAX_PAIRS, PDSC_RANSAC_MAX_N, PDSC_RANSAC_MAX_ITERATIONS);
    const RansacLayout L = ransac_layout(bs, N, I);
    if (workspace_bytes < L.total) {
        set_error("pdsc_ransac_correspondence: workspace %zu bytes < %zu", workspace_bytes, L.total);
        return PDSC_ERR_WORKSPACE;
    }
    unsigned char* ws = (unsigned char*)workspace;
    int* list = (int*)(ws + L.list);
    int* Mv = (int*)(ws + L.m);
    double* pose = hyp_trans ? hyp_trans : (double*)(ws + L.pose);
    int* count = hyp_count ? hyp_count : (int*)(ws + L.count);
    double* sumsq = hyp_sumsq ? hyp_sumsq : (double*)(ws + L.sumsq);
    int* pcount = (int*)(ws + L.pcount);
    double* psumsq = (double*)(ws + L.psumsq);
    // the guards open3d evaluates before its loop; r * r in fp64, and a threshold no d2 can be below when r <= 0 or r is NaN
    const int enabled = r > 0.0 ? 1 : 0;
    const double r2 = enabled ? r * r : 0.0;
    const int tiles = ceil_div(I, RANSAC_NT);
    // stage_ms (pdsc_ransac_correspondence_stages): events around the four launches, read after a host synchronisation
    hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    bool ev_ok = true;
    auto mark = [&](int i) {
        if (stage_ms && ev_ok) ev_ok = hipEventCreate(&ev[i]) == hipSuccess && hipEventRecord(ev[i], st) == hipSuccess;
    };
    mark(0);
    hipLaunchKernelGGL(ransac_compact_kernel, dim3(bs), dim3(RANSAC_SEL_NT), 0, st, mask, counts, list, Mv, N);
    mark(1);
    hipLaunchKernelGGL(ransac_hypothesis_kernel, dim3(tiles, bs), dim3(RANSAC_NT), 0, st, src, tgt, list, Mv, samples, enabled, ransac_n, I,
                       seed, pair_offset, pose, N);
    mark(2);
    hipLaunchKernelGGL(ransac_score_kernel, dim3(tiles, L.split ? L.nchunk : 1, bs), dim3(RANSAC_NT), 0, st, src, tgt, list, Mv, pose, r2,
                       count, sumsq, pcount, psumsq, I, N, L.nchunk, L.split);
    mark(3);
    hipLaunchKernelGGL(ransac_select_kernel, dim3(bs), dim3(RANSAC_SEL_NT), 0, st, src, tgt, list, Mv, pose, r2, count, sumsq, pcount, psumsq,
                       trans, labels, fitness, inlier_rmse, best_iter, num_candidates, I, N, L.nchunk, L.split);
    mark(4);
    int rc = check_launch("pdsc_ransac_correspondence");
    if (stage_ms) {
        if (rc == PDSC_OK) {
            ev_ok = ev_ok && hipEventSynchronize(ev[4]) == hipSuccess;
            for (int i = 0; i < 4 && ev_ok; ++i) ev_ok = hipEventElapsedTime(&stage_ms[i], ev[i], ev[i + 1]) == hipSuccess;
            if (!ev_ok) {
                (void)hipGetLastError();
                set_error("pdsc_ransac_correspondence_stages: event timing failed");
                rc = PDSC_ERR_LAUNCH;
            }
        }
        for (int i = 0; i < 5; ++i)
            if (ev[i]) (void)hipEventDestroy(ev[i]);
    }
    return rc;
}

}  // namespace pdsc

extern "C" size_t pdsc_ransac_workspace_bytes(int bs, int N, int I) { return pdsc::ransac_workspace_bytes(bs, N, I); }

extern "C" int pdsc_ransac_correspondence(const float* src, const float* tgt, const int* counts, const float* mask, const int* samples,
                                          double r, int ransac_n, int max_iteration, unsigned long long seed, long long pair_offset,
                                          float* trans, float* labels, double* fitness, double* inlier_rmse, int* best_iter,
                                          int* num_candidates, double* hyp_trans, int* hyp_count, double* hyp_sumsq, void* workspace,
                                          size_t workspace_bytes, int bs, int N, void* stream) {
    return pdsc::launch_ransac_correspondence(src, tgt, counts, mask, samples, r, ransac_n, max_iteration, seed, pair_offset, trans, labels,
                                              fitness, inlier_rmse, best_iter, num_candidates, hyp_trans, hyp_count, hyp_sumsq, workspace,
                                              workspace_bytes, bs, N, (hipStream_t)stream, nullptr);
}

extern "C" int pdsc_ransac_correspondence_stages(const float* src, const float* tgt, const int* counts, const float* mask,
                                                 const int* samples, double r, int ransac_n, int max_iteration, unsigned long long seed,
                                                 long long pair_offset, float* trans, float* labels, double* fitness, double* inlier_rmse,
                                                 int* best_iter, int* num_candidates, double* hyp_trans, int* hyp_count, double* hyp_sumsq,
                                                 void* workspace, size_t workspace_bytes, int bs, int N, float* stage_ms, void* stream) {
    if (!stage_ms) {
        pdsc::set_error("pdsc_ransac_correspondence_stages: stage_ms == NULL");
        return PDSC_ERR_ARG;
    }
    return pdsc::launch_ransac_correspondence(src, tgt, counts, mask, samples, r, ransac_n, max_iteration, seed, pair_offset, trans, labels,
                                              fitness, inlier_rmse, best_iter, num_candidates, hyp_trans, hyp_count, hyp_sumsq, workspace,
                                              workspace_bytes, bs, N, (hipStream_t)stream, stage_ms);
}
