// f-13: backward of the feature-similarity matrix M = clamp(1 - (1 - F F^T) / sigma^2, 0, 1), zero diagonal (pdsc_feature_compat,
// models/PointDSC.py:160-163) for an ARBITRARY upstream gradient dM [bs][N][ld] -- what loss.backward() needs to reach the weights
// through res['M'] of the train-mode forward.  A sibling of sm_loss_features_kernel<true> (losses.hip), where the loss's own
// coefficient stands in place of dM:
//   live_ij = (i != j) and 0 <= raw_ij <= 1 (inclusive: torch.clamp's backward),   g_ij = live_ij ? dM_ij : 0
//   dF_i    = (1 / sigma^2) sum_j (g_ij + g_ji) F_j
//   dsigma  = (2 / sigma^3) sum_b sum_ij g_ij (1 - s_ij)
// Determinism: no floating-point atomics.  A workgroup owns 128 rows i (a wavefront 32 of them, lane & 31) and walks 32-index
// tiles of the other index o, so every dF_i has one writer and one order; dsigma goes through fp64 partials (one per workgroup,
// fixed tree) that a finishing launch adds in index order.
//
// Element order and arithmetic are those of losses.hip: per tile a lane holds the 16 elements o = tile * 32 + (r & 3) + 8 (r >> 2)
// + 4 (lane >> 5) -- the accumulator layout of v_mfma_f32_32x32x2_f32 -- of s(i, o) = <F_i, F_o>, computed by gram_tile_k128 with
// the tile's rows F_o as the A operand and the wave's own rows F_i as the B operand, and raw = feature_compat_raw(s, sigma^2):
// the text pdsc_feature_compat stores M[o][i] with.  The same s decides live_io: the roles of the two rows are swapped there, which
// swaps the factors of every product (IEEE multiplication commutes) and leaves the k order as it is, so M is symmetric bit for bit
// (tests/test_feature_compat_backward.py asserts that on the matrix the forward writes).
//
// dM is NOT assumed symmetric, so a tile needs dM[i][o] and dM[o][i]:
//   dM[o][i]: lane = i, register = o -- a half wave reads 128 contiguous bytes of row o, straight into the accumulator layout;
//   dM[i][o]: read as rows too (lane & 31 = o, 128 contiguous bytes of row i), and transposed through a wave-private LDS tile.
// Every value that must not count -- dead entries, the diagonal, tail rows and columns, the pad columns [N, ld) -- is SELECTED to 0
// (never multiplied by 0, never loaded where it lies outside the matrix): a NaN or inf there does not leak.
// The gradient tile g(i, o) + g(o, i) is then ALREADY the A operand of the second product dF_i += sum_o (.) F_o (k slot (step r,
// half h) <-> o), exact fp32 on v_mfma_f32_32x32x2_f32 with the staged tile as the B operand, as in losses.hip.
#include "pdsc_common.h"
#include "gram_tile.h"

namespace pdsc {

constexpr int FCB_ROWS = 128, FCB_TILE = 32, FCB_LD = PDSC_CHANNELS + 4, FCB_TLD = FCB_TILE + 1;
constexpr size_t FCB_LDS_BYTES = (2 * (size_t)FCB_TILE * FCB_LD + 4 * (size_t)FCB_TILE * FCB_TLD) * sizeof(float);      // 50 688 B

struct FcbArgs {
    const float* X;          // [bs][N][128]
    const float* sigma;
    const float* dM;         // [bs][N][ld]
    long long ld;
    double* part;            // [bs][row blocks]: sum over the workgroup's rows i and all o of g_io (1 - s_io)
    float* dnormed;          // [bs][N][128] or NULL
    int N;
};

__global__ __launch_bounds__(256) void feature_compat_backward_kernel(FcbArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];       // 2 x [FCB_TILE][FCB_LD] feature tiles, 4 x [FCB_TILE][FCB_TLD] dM tiles
    __shared__ double red[4];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, l31 = lane & 31, h = lane >> 5;
    const int b = blockIdx.y, rb = blockIdx.x, N = a.N;
    const long long ld = a.ld;
    const float* X = a.X + (size_t)b * N * PDSC_CHANNELS;
    const float* G = a.dM + (size_t)b * N * ld;
    const float sg = a.sigma[0], sig2 = sg * sg;
    const bool want_df = a.dnormed != nullptr;

    // this lane's own row: B fragments, k-slot (4q+e, half h) <-> channel 8q+4h+e (the convention of linear.hip)
    const int i = rb * FCB_ROWS + wave * 32 + l31;
    const bool vi = i < N;
    f32x4 bf[16];
    {
        const float* p = X + (size_t)min(i, N - 1) * PDSC_CHANNELS + 4 * h;
#pragma unroll
        for (int q = 0; q < 16; ++q) bf[q] = *reinterpret_cast<const f32x4*>(p + 8 * q);
    }
    // stage loader: thread -> 4 float4 of a 32 x 128 tile (rows past N repeat row N - 1: finite values under a zero gradient)
    f32x4 stage[4];
    auto load_tile = [&](int tile) {
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int f = t + 256 * s, r = f >> 5, c4 = (f & 31) * 4;
            const int col = min(tile * FCB_TILE + r, N - 1);
            stage[s] = *reinterpret_cast<const f32x4*>(X + (size_t)col * PDSC_CHANNELS + c4);
        }
    };
    auto store_tile = [&](float* buf) {
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int f = t + 256 * s, r = f >> 5, c4 = (f & 31) * 4;
            *reinterpret_cast<f32x4*>(buf + r * FCB_LD + c4) = stage[s];
        }
    };
    // dM[i-tile][o-tile] of this wave's 32 rows: register r of lane (l31, h) is row 2 r + h, column l31 -- a half wave reads 128
    // contiguous bytes of one row; nothing outside the N x N matrix is read
    float tstage[16];
    auto load_dmt = [&](int tile) {
        const int o = tile * FCB_TILE + l31;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = rb * FCB_ROWS + wave * 32 + 2 * r + h;
            tstage[r] = 0.f;
            if (row < N && o < N) tstage[r] = G[(size_t)row * ld + o];
        }
    };
    float* T = lds + 2 * FCB_TILE * FCB_LD + wave * FCB_TILE * FCB_TLD;      // wave-private: only this wave writes and reads it
    auto store_dmt = [&]() {
#pragma unroll
        for (int r = 0; r < 16; ++r) T[(2 * r + h) * FCB_TLD + l31] = tstage[r];
    };
    f32x16 dF[4];                                   // 32 rows x 128 channels of sum_o (g_io + g_oi) F_o, 4 accumulator tiles
#pragma unroll
    for (int cb = 0; cb < 4; ++cb)
#pragma unroll
        for (int r = 0; r < 16; ++r) dF[cb][r] = 0.f;
    double dsg = 0.0;
    const int tiles = ceil_div_dev(N, FCB_TILE);
    load_tile(0);
    load_dmt(0);
    store_tile(lds);
    store_dmt();
    __syncthreads();
    for (int tile = 0; tile < tiles; ++tile) {
        const float* cur = lds + (tile & 1) * FCB_TILE * FCB_LD;
        // this tile's dM[i][o] out of the transpose tile (one buffer: the wave overwrites it at the bottom of this iteration, after
        // these reads in its own program order) and dM[o][i] from memory
        float gio[16], goi[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int ol = (r & 3) + 8 * (r >> 2) + 4 * h, o = tile * FCB_TILE + ol;
            gio[r] = T[l31 * FCB_TLD + ol];
            goi[r] = 0.f;
            if (vi && o < N) goi[r] = G[(size_t)o * ld + i];
        }
        __builtin_amdgcn_wave_barrier();
        if (tile + 1 < tiles) {                                          // in flight under the MFMAs
            load_tile(tile + 1);
            load_dmt(tile + 1);
        }
        const f32x16 acc = gram_tile_k128<false>(bf, cur + l31 * FCB_LD + 4 * h);      // gram_tile.h: A = the tile's rows, B = own rows
        float g[16];
        float dsg_tile = 0.f;                       // fp32 over the 16 elements of one tile column, fp64 above
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int o = tile * FCB_TILE + (r & 3) + 8 * (r >> 2) + 4 * h;
            const float s = acc[r];
            const float raw = feature_compat_raw(s, sig2);
            const bool live = vi && o < N && i != o && raw >= 0.0f && raw <= 1.0f;       // inclusive: torch.clamp's backward
            const float g_io = live ? gio[r] : 0.0f, g_oi = live ? goi[r] : 0.0f;
            g[r] = g_io + g_oi;
            dsg_tile += g_io * (1.0f - s);
        }
        dsg += (double)dsg_tile;
        if (want_df) {
            // dF[i][c] += sum_o g(i, o) F_o[c]: A = g straight from the registers (lane = i, k slot (r, h) <-> o), B = the staged tile
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float* frow = cur + ((r & 3) + 8 * (r >> 2) + 4 * h) * FCB_LD + l31;
#pragma unroll
                for (int cb = 0; cb < 4; ++cb) dF[cb] = __builtin_amdgcn_mfma_f32_32x32x2f32(g[r], frow[32 * cb], dF[cb], 0, 0, 0);
            }
        }
        if (tile + 1 < tiles) {
            store_tile(lds + ((tile + 1) & 1) * FCB_TILE * FCB_LD);      // the other buffer: its readers finished a barrier ago
            store_dmt();
            __syncthreads();
        }
    }
    if (want_df) {
        const float scale = 1.0f / sig2;
        float* D = a.dnormed + (size_t)b * N * PDSC_CHANNELS;
#pragma unroll
        for (int cb = 0; cb < 4; ++cb)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = rb * FCB_ROWS + wave * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;       // accumulator lane = channel
                if (row < N) D[(size_t)row * PDSC_CHANNELS + 32 * cb + l31] = scale * dF[cb][r];
            }
    }
    // the workgroup's fp64 partial: wave shuffle tree, then the waves in order
    dsg = wave_sum(dsg);
    if (lane == 0) red[wave] = dsg;
    __syncthreads();
    if (t == 0) a.part[(size_t)b * gridDim.x + rb] = ((red[0] + red[1]) + red[2]) + red[3];
}

// dsigma = (2 / sigma^3) * the partials added in index order
__global__ __launch_bounds__(64) void feature_compat_backward_finish_kernel(const double* __restrict__ part, int count,
                                                                            const float* __restrict__ sigma, double* __restrict__ dsigma) {
    if (threadIdx.x != 0) return;
    double d = 0.0;
    for (int p = 0; p < count; ++p) d += part[p];
    const double sg = (double)sigma[0];
    dsigma[0] = d * 2.0 / (sg * sg * sg);
}

}  // namespace pdsc

extern "C" size_t pdsc_feature_compat_backward_workspace_bytes(int bs, int N) {
    if (bs <= 0 || N <= 0) return 0;
    return (size_t)bs * pdsc::ceil_div(N, pdsc::FCB_ROWS) * sizeof(double);
}

extern "C" int pdsc_feature_compat_backward(const float* normed, const float* sigma, const float* dM, long long ld, float* dnormed,
                                            double* dsigma, void* ws, size_t ws_bytes, int bs, int N, void* stream) {
    PDSC_REQUIRE(normed && sigma && dM, "pdsc_feature_compat_backward: null pointer");
    PDSC_REQUIRE(dnormed || dsigma, "pdsc_feature_compat_backward: neither gradient asked for");
    PDSC_REQUIRE(bs > 0 && N > 0 && bs <= 65535 && ld >= N, "pdsc_feature_compat_backward: bs=%d N=%d ld=%lld", bs, N, ld);
    PDSC_REQUIRE(((uintptr_t)normed & 15) == 0 && (!dnormed || ((uintptr_t)dnormed & 3) == 0),
                 "pdsc_feature_compat_backward: normed must be 16-byte aligned");
    PDSC_REQUIRE(ws && ((uintptr_t)ws & 7) == 0, "pdsc_feature_compat_backward: workspace must be 8-byte aligned");
    if (ws_bytes < pdsc_feature_compat_backward_workspace_bytes(bs, N)) {
        pdsc::set_error("pdsc_feature_compat_backward: workspace of %zu bytes, needs %zu", ws_bytes,
                        pdsc_feature_compat_backward_workspace_bytes(bs, N));
        return PDSC_ERR_WORKSPACE;
    }
    hipStream_t st = (hipStream_t)stream;
    const int rc_lds = pdsc::ensure_dynamic_lds(reinterpret_cast<const void*>(&pdsc::feature_compat_backward_kernel), pdsc::FCB_LDS_BYTES,
                                                "feature_compat_backward(dynamic LDS)");
    if (rc_lds != PDSC_OK) return rc_lds;
    const int rbs = pdsc::ceil_div(N, pdsc::FCB_ROWS);
    pdsc::FcbArgs a{};
    a.X = normed; a.sigma = sigma; a.dM = dM; a.ld = ld; a.part = (double*)ws; a.dnormed = dnormed; a.N = N;
    hipLaunchKernelGGL(pdsc::feature_compat_backward_kernel, dim3(rbs, bs), dim3(256), pdsc::FCB_LDS_BYTES, st, a);
    if (dsigma)
        hipLaunchKernelGGL(pdsc::feature_compat_backward_finish_kernel, dim3(1), dim3(64), 0, st, (const double*)ws, bs * rbs, sigma, dsigma);
    return pdsc::check_launch("pdsc_feature_compat_backward");
}
