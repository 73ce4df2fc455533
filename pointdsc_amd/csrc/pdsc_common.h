// Shared host/device helpers for libpointdsc_hip.so (gfx950 only: wave64, MFMA, 160 KiB LDS).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include "../../include/pointdsc_hip.h"

#define PDSC_WAVE 64

// the 16-bit element of every split-precision ("x3") operand -- hi or lo part of an fp32 value, split_layout.h -- and the matrix
// instruction that multiplies them
typedef _Float16 sp16;
typedef sp16 sp16x2 __attribute__((ext_vector_type(2)));
typedef sp16 sp16x4 __attribute__((ext_vector_type(4)));
typedef sp16 sp16x8 __attribute__((ext_vector_type(8)));
#define PDSC_MFMA_X3 __builtin_amdgcn_mfma_f32_32x32x16_f16

namespace pdsc {

// ---- host-side error plumbing ---------------------------------------------------------------
void set_error(const char* fmt, ...);
int check_launch(const char* what);

#define PDSC_REQUIRE(cond, ...)                       \
    do {                                              \
        if (!(cond)) {                                \
            pdsc::set_error(__VA_ARGS__);             \
            return PDSC_ERR_ARG;                      \
        }                                             \
    } while (0)

// Dynamic-LDS opt-in (hipFuncAttributeMaxDynamicSharedMemorySize) of kernel `fn`, done once per (kernel, device) --
// the attribute is per device -- and checked: returns PDSC_OK or PDSC_ERR_LAUNCH with the error text set.  Thread-safe.
int ensure_dynamic_lds(const void* fn, size_t bytes, const char* what);

// buffer := value, as a kernel launch on `st` (NOT hipMemsetAsync: profiles/r03_p_diverge_probe.txt -- with several forwards in
// flight, and above all inside replayed hipGraphs, the zeroing of the hypothesis counters was not reliably ordered before the
// scoring kernel's atomicAdds that follow it on the same stream; a kernel node is)
int launch_fill_u32(unsigned int* p, unsigned int value, size_t count, hipStream_t st);
int launch_copy_u32(unsigned int* dst, const unsigned int* src, size_t count, hipStream_t st);      // dst[i] = src[i], likewise a kernel
// linear.hip: the first two layers of the confidence head in one launch (bit-identical to two pdsc_linear launches)
int launch_classifier_hidden(const float* X, const float* W1, const float* b1, const float* W2, const float* b2, float* H2, int M,
                             hipStream_t st);

// fp16 range sentinel (r06): the split-precision arithmetic carries activations as fp16 hi + lo pairs, so |x| must stay below 65504.
// Every site that converts an activation notes its magnitude (range_note: one v_max3_f32 per two values); a wavefront whose maximum
// reaches the bound sets the word of its pair in `range_flag` ([bs] u32, workspace entry "range_flag": zeroed by the forward's first
// launch, read by its last one, which turns the pose of such a pair into NaN -- a result that is wrong is never returned silently).
// run_forward passes the array to EVERY fused-layer launch in LayerArgs.range_flag (layer_args.h: which kernels note what, and the
// three experiments-only paths that carry no sentinel: generic H3 wave form, layer_split.hip, PDSC_FUSED_LAYERS = 0), and the
// validation forward, which has no refinement launch, turns the flagged poses into NaN in a launch of its own; stage-level calls
// outside a forward leave it NULL and the kernels skip the report.
constexpr float PDSC_F16_RANGE = 65504.0f;

// opt-in event timing of the roofline kernels (api.hip); no-ops unless pdsc_profile_enable() was called
void profile_mark_begin(int kind, hipStream_t st);
void profile_mark_end(int kind, hipStream_t st);

// Tuning / A-B knobs (PDSC_* environment variables, listed in DESIGN.md) exist in EXPERIMENTS builds only
// (-DPDSC_EXPERIMENTS: libpointdsc_hip_exp.so, built by `python -m pointdsc_amd.build --experiments` for tools/ab_*.py).  In
// the product library env_int / env_str return the default without looking at the environment: nothing outside
// pdsc_config can change what a drop-in module computes or which kernel it runs.
#ifdef PDSC_EXPERIMENTS
static inline int env_int(const char* name, int dflt) {
    const char* e = getenv(name);
    return e ? atoi(e) : dflt;
}
static inline const char* env_str(const char* name) { return getenv(name); }
#else
static inline int env_int(const char*, int dflt) { return dflt; }
static inline const char* env_str(const char*) { return nullptr; }
#endif

// The smallest fp32 x with sqrtf(x) >= thr (host sqrtf is correctly rounded, like the device's): since the correctly
// rounded square root is monotone, `sqrt(x) >= thr` <=> `x >= x*` and `sqrt(x) < thr` <=> `x < x*`, bit for bit -- lets
// the N^2 / S*N predicate loops compare the radicand and skip the ~20-instruction IEEE sqrt.  thr <= 0 -> 0; NaN -> NaN.
static inline float sqrt_threshold_radicand(float thr) {
    float x = 0.f;
    if (thr > 0.f) {
        x = thr * thr;
        while (x > 0.f && sqrtf(nextafterf(x, 0.f)) >= thr) x = nextafterf(x, 0.f);
        while (sqrtf(x) < thr) x = nextafterf(x, INFINITY);
    } else if (thr != thr) {
        x = thr;
    }
    return x;
}

static inline long long round_up(long long x, long long m) { return (x + m - 1) / m * m; }
static inline int ceil_div(int a, int b) { return (a + b - 1) / b; }
__device__ __forceinline__ int ceil_div_dev(int a, int b) { return (a + b - 1) / b; }

// ---- device helpers ----------------------------------------------------------------------------
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

// running maximum of |x| over the values a lane converts to fp16: ONE v_max3_f32 per two values (|abs| source modifiers; v_max ignores
// NaN operands: a NaN input is not an overflow and propagates on its own, as it does in the reference).  The values are in/out operands
// of the statement although it does not change them: the conversion that follows then depends on it, so the scheduler cannot sink the
// note past the point where the fp32 values die (as plain fmaxf calls it sank them to the end of the pinned pipelines of layer_h3.hip
// and kept every fp32 source alive: 295 spilled registers).
__device__ __forceinline__ void range_note(float& r, float& x0, float& x1) {
    asm("v_max3_f32 %0, %0, |%1|, |%2|" : "+v"(r), "+v"(x0), "+v"(x1));
}
__device__ __forceinline__ void range_note(float& r, f32x4& v) {
    asm("v_max3_f32 %0, %0, |%1|, |%2|" : "+v"(r), "+v"(v[0]), "+v"(v[1]));
    asm("v_max3_f32 %0, %0, |%1|, |%2|" : "+v"(r), "+v"(v[2]), "+v"(v[3]));
}
// end of a wavefront's work: one store per wavefront and only when the bound was reached (all writers store the same value)
__device__ __forceinline__ void range_report(unsigned int* flag, int pair, float r) {
    if (flag && __builtin_amdgcn_ballot_w64(!(r < PDSC_F16_RANGE)) != 0ull && (threadIdx.x & 63) == 0) flag[pair] = 1u;
}

// Euclidean norm of a 3-vector with torch's CPU/GPU reduction order: sqrt(fma(z,z,fma(y,y,x*x))).
// (oracle/pointdsc_oracle.py:pairwise_dist documents the measurement.)  sqrtf is IEEE-correct
// (hipcc default -fhip-fp32-correctly-rounded-divide-sqrt).
__device__ __forceinline__ float norm3(float x, float y, float z) {
    return sqrtf(fmaf(z, z, fmaf(y, y, x * x)));
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}
__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}
// Wave-wide float sum on the VALU's data-parallel primitives (DPP) instead of six ds_bpermute round trips through the LDS
// crossbar (~100 cycles each): pair swap, quad swap, half-row mirror, row mirror leave every lane of a 16-lane row with
// the row total (both partners of every step add the same two numbers, so the copies are bit-identical); row_bcast:15 /
// row_bcast:31 fold the four rows into lane 63; one v_readlane broadcasts.  Deterministic, but ANOTHER summation order than
// wave_sum above -- used where a wavefront owns a whole small problem (per-seed solver), not where bit patterns are pinned.
__device__ __forceinline__ float wave_sum_dpp(float v) {
#define PDSC_DPP_ADD(ctrl, row_mask)                                                                                    \
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), ctrl, row_mask, 0xf, false))
    PDSC_DPP_ADD(0xB1, 0xf);      // quad_perm [1,0,3,2]
    PDSC_DPP_ADD(0x4E, 0xf);      // quad_perm [2,3,0,1]
    PDSC_DPP_ADD(0x141, 0xf);     // row_half_mirror
    PDSC_DPP_ADD(0x140, 0xf);     // row_mirror
    PDSC_DPP_ADD(0x142, 0xa);     // row_bcast:15 -> rows 1, 3
    PDSC_DPP_ADD(0x143, 0xc);     // row_bcast:31 -> rows 2, 3
#undef PDSC_DPP_ADD
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 63));
}

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
    return v;
}

// Block-wide sum of NV floats per thread; result valid in every thread.  `red` needs NV*nwaves floats.
template <int NV, int NWAVES>
__device__ __forceinline__ void block_sum(float (&v)[NV], float* red) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < NV; ++i) v[i] = wave_sum(v[i]);
    __syncthreads();  // protect `red` from the previous use
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < NV; ++i) red[wave * NV + i] = v[i];
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        float s = 0.f;
#pragma unroll
        for (int w = 0; w < NWAVES; ++w) s += red[w * NV + i];
        v[i] = s;
    }
}

// ---- the 3x3 fp64 core: jacobi_eig3, kabsch_from_covariance (fp32), kabsch_from_covariance_f64, ssb_kabsch (the backward's) ----
#define PDSC_COMMON_INCLUDES_KABSCH3
#include "kabsch3.h"
#undef PDSC_COMMON_INCLUDES_KABSCH3

// ---- exact fp32 sqrt / divide-by-invariant without the compiler's special-case scaffolding --------------
// sqrt: hipcc lowers a correctly rounded sqrtf to v_sqrt_f32 followed by exactly this one-ulp test (plus input
// scaling below 2^-96 and a zero/inf class check).  For x == 0 both residual tests fail and 0 is returned.
__device__ __forceinline__ float sqrt_rn(float x) {
    float s = __builtin_amdgcn_sqrtf(x);
    const float sd = __uint_as_float(__float_as_uint(s) - 1u);
    const float su = __uint_as_float(__float_as_uint(s) + 1u);
    const float rd = fmaf(-sd, s, x);
    const float ru = fmaf(-su, s, x);
    s = rd <= 0.0f ? sd : s;
    s = ru > 0.0f ? su : s;
    return s;
}

}  // namespace pdsc
