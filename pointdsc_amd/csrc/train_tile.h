// The fp32-MFMA tile of the train path (f-17): what pointwise_train.hip (conv + batch-norm + ReLU) and linear_train.hip (layer0, q|k|v,
// fc_message.6, head) share, once.  All products run on v_mfma_f32_32x32x2_f32 (exact fp32 products, one rounding per accumulate) over
// 64-row tiles whose whole K sits in LDS behind linear.hip's row pad of 4.  Operand convention wherever a lane's four k values are
// contiguous in LDS: k-slot (step 4q+e, half h = lane>>5) <-> channel 8q+4h+e.  The backward's parameter gradients are accumulated in
// registers by persistent workgroups (at most TT_MAX_GROUPS) over the tiles they walk, written as one partial per workgroup
// (tt_write_dw_blocks, tt_column_sums) and added in index order by tt_merge_kernel: no atomics, no memset, nothing allocated, every sum
// in a fixed order -- repeat calls give the same bits, and so do the kernels of the two files, which run the SAME loops below.
// Every kernel built on the device pieces has 256 threads (4 waves); the merge kernel has TT_MERGE_THREADS.
#pragma once
#include "pdsc_common.h"

namespace pdsc {

constexpr int TT_BM = 64;                  // rows per tile
constexpr int TT_PAD = 4;                  // floats behind every staged row
constexpr int TT_MAX_GROUPS = 256;         // persistent workgroups of the backward kernels: one per compute unit
constexpr int TT_MERGE_THREADS = 1024;

static int tt_tiles(int M) { return ceil_div(M, TT_BM); }
static int tt_groups(int M) { const int t = tt_tiles(M); return t < TT_MAX_GROUPS ? t : TT_MAX_GROUPS; }

// ---- accumulators --------------------------------------------------------------------------------------------------------------
template <int N>
__device__ __forceinline__ void tt_zero(f32x16 (&acc)[N]) {
#pragma unroll
    for (int i = 0; i < N; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;
}
// row of a 32 x 32 block that register r of half h holds (its column is lane & 31)
__device__ __forceinline__ int tt_acc_row(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

// ---- staging: rows row0 .. row0 + rows - 1 of src [..][C] -> LDS [rows][C + TT_PAD], rows >= nvalid zero -------------------------
// (base pointer and first row apart: a pre-offset pointer costs the dW-accumulating kernels 16 VGPRs)
template <int C>
__device__ __forceinline__ void tt_stage_rows16(const float* __restrict__ src, int row0, float* dst, int rows, int nvalid) {
    constexpr int LD = C + TT_PAD, K4 = C / 4;
    for (int idx = threadIdx.x; idx < rows * K4; idx += 256) {
        const int row = idx / K4, c = idx - row * K4;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (row < nvalid) v = *reinterpret_cast<const f32x4*>(src + (size_t)(row0 + row) * C + c * 4);
        *reinterpret_cast<f32x4*>(dst + row * LD + c * 4) = v;
    }
}
// the scalar form for rows of Cin <= CS floats (no alignment asked of them): columns Cin .. CS - 1 zero as well
template <int CS>
__device__ __forceinline__ void tt_stage_rows_scalar(const float* __restrict__ src, int row0, float* dst, int rows, int nvalid, int Cin) {
    constexpr int LD = CS + TT_PAD;
    for (int idx = threadIdx.x; idx < rows * CS; idx += 256) {
        const int row = idx / CS, c = idx - row * CS;
        dst[row * LD + c] = (row < nvalid && c < Cin) ? src[(size_t)(row0 + row) * Cin + c] : 0.f;
    }
}
// CS >= 64: Cin == CS, 16-byte form
template <int CS>
__device__ __forceinline__ void tt_stage_rows(const float* __restrict__ src, int row0, float* dst, int rows, int nvalid, int Cin) {
    if (CS >= 64) tt_stage_rows16<CS>(src, row0, dst, rows, nvalid);
    else tt_stage_rows_scalar<CS>(src, row0, dst, rows, nvalid, Cin);
}

// ---- the three products; acc[i] is a wave's i-th 32 x 32 block, UNROLL the unroll factor of the k loop ---------------------------
// rows x rows, C = A B^T:  A = the wave's 32 rows [32][lda], B = its NT * 32 rows [..][ldb], k = channel, 0 .. K - 1 (both operands
// one 16-byte read per four steps).  RELU_A: relu on A as it is read.
template <int K, int NT, int UNROLL, bool RELU_A = false>
__device__ __forceinline__ void tt_mma_rows_rows(const float* A, int lda, const float* B, int ldb, f32x16 (&acc)[NT]) {
    const int l31 = threadIdx.x & 31, h = (threadIdx.x >> 5) & 1;
    const float* xa = A + l31 * lda + 4 * h;
    const float* wb = B + l31 * ldb + 4 * h;
#pragma unroll UNROLL
    for (int q = 0; q < K / 8; ++q) {
        const f32x4 av = *reinterpret_cast<const f32x4*>(xa + 8 * q);
        f32x4 bv[NT];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) bv[nt] = *reinterpret_cast<const f32x4*>(wb + nt * 32 * ldb + 8 * q);
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
                acc[nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(RELU_A ? fmaxf(av[e], 0.f) : av[e], bv[nt][e], acc[nt], 0, 0, 0);
    }
}
// rows x columns, C = A B:  A = the wave's 32 rows [32][lda] (k = its channel; 16-byte reads), B = [K][ldb] from the first of the wave's
// NT * 32 columns on, read down a column
template <int K, int NT, int UNROLL>
__device__ __forceinline__ void tt_mma_rows_cols(const float* A, int lda, const float* B, int ldb, f32x16 (&acc)[NT]) {
    const int l31 = threadIdx.x & 31, h = (threadIdx.x >> 5) & 1;
    const float* ya = A + l31 * lda + 4 * h;
    const float* wb = B + (4 * h) * ldb + l31;
#pragma unroll UNROLL
    for (int q = 0; q < K / 8; ++q) {
        const f32x4 av = *reinterpret_cast<const f32x4*>(ya + 8 * q);
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
                acc[nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[e], wb[(8 * q + e) * ldb + nt * 32], acc[nt], 0, 0, 0);
    }
}
// columns x columns, C += A^T B over the K rows of a tile:  A [K][lda], B [K][ldb], k = row 2 step + h, both operands one 4-byte read
// per step.  The wave's blocks are j = j0 .. j0 + TPW - 1 of the CIB-wide grid: block (j / CIB) of A's columns x block (j % CIB) of
// B's.  RELU_B: relu on B as it is read.
template <int K, int TPW, int CIB, int UNROLL, bool RELU_B = false>
__device__ __forceinline__ void tt_mma_cols_cols(const float* A, int lda, const float* B, int ldb, int j0, f32x16 (&acc)[TPW]) {
    const int l31 = threadIdx.x & 31, h = (threadIdx.x >> 5) & 1;
#pragma unroll UNROLL
    for (int st = 0; st < K / 2; ++st) {
        const float* yr = A + (2 * st + h) * lda + l31;
        const float* xr = B + (2 * st + h) * ldb + l31;
#pragma unroll
        for (int i = 0; i < TPW; ++i) {
            const int j = j0 + i;
            const float bv = xr[(j % CIB) * 32];
            acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(yr[(j / CIB) * 32], RELU_B ? fmaxf(bv, 0.f) : bv, acc[i], 0, 0, 0);
        }
    }
}

// ---- a workgroup's partial ---------------------------------------------------------------------------------------------------------
// the blocks of tt_mma_cols_cols -> P [rows of A's columns][ldp], columns >= ncols not written
template <int TPW, int CIB>
__device__ __forceinline__ void tt_write_dw_blocks(float* P, int ldp, int ncols, int j0, const f32x16 (&acc)[TPW]) {
    const int l31 = threadIdx.x & 31, h = (threadIdx.x >> 5) & 1;
#pragma unroll
    for (int i = 0; i < TPW; ++i) {
        const int j = j0 + i;
        const int ci = (j % CIB) * 32 + l31;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int co = (j / CIB) * 32 + tt_acc_row(r, h);
            if (ci < ncols) P[(size_t)co * ldp + ci] = acc[i][r];
        }
    }
}
// Column sums over the RL row lanes, in order.  Row lane rl holds v[e], its part of column col0 + e * stride; -> thread t < NCOL the
// sum of column t (other threads 0).  red: RL * NCOL floats of LDS that nobody reads any more; begins and ends with a barrier inside.
template <int RL, int NCOL>
__device__ __forceinline__ float tt_column_sums(float* red, const float (&v)[4], int rl, int col0, int stride) {
    __syncthreads();
#pragma unroll
    for (int e = 0; e < 4; ++e) red[rl * NCOL + col0 + e * stride] = v[e];
    __syncthreads();
    float s = 0.f;
    if (threadIdx.x < NCOL) {
#pragma unroll
        for (int j = 0; j < RL; ++j) s += red[j * NCOL + threadIdx.x];
    }
    return s;
}

// ---- the workgroups' partials in index order -> the caller's tensors -----------------------------------------------------------------
// part [sets = gridDim.y][groups][total]; element el of set y goes to the segment k with set[k] == y and begin[k] <= el < end[k]
// (a NULL out[k]: not wanted).  thread = (slice, element), 16 slices x 64 elements.
constexpr int TT_MAX_SEGS = 6;
struct TtMergeSegs {
    int set[TT_MAX_SEGS], begin[TT_MAX_SEGS], end[TT_MAX_SEGS];
    float* out[TT_MAX_SEGS];
    int n = 0;
    void add(int s, int b, int e, float* o) { set[n] = s; begin[n] = b; end[n] = e; out[n] = o; ++n; }
};

// (inline: one definition for the two translation units that include this header; the diagnostic only says that nvcc would not honour it)
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wcuda-compat"
inline __global__ __launch_bounds__(TT_MERGE_THREADS) void tt_merge_kernel(const float* __restrict__ part, int groups, int total,
                                                                          TtMergeSegs sg) {
#pragma clang diagnostic pop
    __shared__ float red[TT_MERGE_THREADS];
    const int t = threadIdx.x, el = blockIdx.x * 64 + (t & 63), s = t >> 6, y = blockIdx.y;
    const float* base = part + (size_t)y * groups * total;
    float acc = 0.f;
    if (el < total)
        for (int p = s; p < groups; p += 16) acc += base[(size_t)p * total + el];
    red[t] = acc;
    __syncthreads();
    if (s == 0 && el < total) {
        float tot = 0.f;
#pragma unroll
        for (int j = 0; j < 16; ++j) tot += red[j * 64 + (t & 63)];
#pragma unroll
        for (int k = 0; k < TT_MAX_SEGS; ++k)
            if (k < sg.n && sg.set[k] == y && el >= sg.begin[k] && el < sg.end[k] && sg.out[k]) sg.out[k][el - sg.begin[k]] = tot;
    }
}

static int tt_launch_merge(const float* part, int groups, int total, int sets, const TtMergeSegs& sg, hipStream_t st, const char* what) {
    hipLaunchKernelGGL(tt_merge_kernel, dim3(ceil_div(total, 64), sets), dim3(TT_MERGE_THREADS), 0, st, part, groups, total, sg);
    return check_launch(what);
}

// ---- host side -----------------------------------------------------------------------------------------------------------------------
// dynamic-LDS opt-in, launch with 256 threads, check
template <class Args>
static int launch_with_dynamic_lds(void (*kernel)(Args), dim3 grid, size_t lds_bytes, hipStream_t st, const char* what, const Args& a) {
    char attr[96];
    snprintf(attr, sizeof(attr), "%s(dynamic LDS)", what);
    const int rc = ensure_dynamic_lds(reinterpret_cast<const void*>(kernel), lds_bytes, attr);
    if (rc != PDSC_OK) return rc;
    hipLaunchKernelGGL(kernel, grid, dim3(256), lds_bytes, st, a);
    return check_launch(what);
}

static int check_workspace(const char* what, size_t have, size_t need) {
    if (have >= need) return PDSC_OK;
    set_error("%s: workspace of %zu bytes, needs %zu", what, have, need);
    return PDSC_ERR_WORKSPACE;
}

static bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace pdsc
