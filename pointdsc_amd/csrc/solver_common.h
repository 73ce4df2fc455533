// What the per-seed solver (solver.hip) and its backward (seed_solve_backward.hip) share: the backward replays the iterate the
// forward chose, with the forward's wave-private LDS hand-over.
#pragma once
#include "pdsc_common.h"

namespace pdsc {

// chosen iterate = first iteration at which EVERY seed of the pair passed allclose (the reference breaks
// there), else the last one.
__device__ __forceinline__ int chosen_iterate(unsigned int mask, int num_iter) {
    const unsigned int m = num_iter >= 32 ? mask : (mask & ((1u << num_iter) - 1u));
    return m ? (__ffs((int)m) - 1) : (num_iter - 1);
}

// LDS written by some lanes of a wavefront becomes visible to all of them (a workgroup here is independent wavefronts: no barrier)
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

}  // namespace pdsc
