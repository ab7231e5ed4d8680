// Device helpers of the row softmax contract (csrc/softmax_kernels.hpp, csrc/attention_kernels.hpp): the wave maximum,
// the row maximum with its NaN rule, the exponential and the final division, each one IEEE fp32 operation per step.
// Helpers only - no kernel is defined here - so the one-pass attention units include it without the softmax kernels.
#pragma once

#include <hip/hip_runtime.h>
#include <math.h>

namespace bsmr {

__device__ __forceinline__ float smWaveMax(float m) {
    for (int o = 32; o; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    return m;
}

// the wave's LDS writes before its own reads (rocPRIM's wave_barrier idiom; the short kernels' waves leave early, so
// no block barrier there)
__device__ __forceinline__ void smWaveSync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// m as the contract defines it: NaN if any z is NaN, else the max
__device__ __forceinline__ float smRowMax(float m, bool nan) { return nan ? __int_as_float(0x7FC00000) : m; }

__device__ __forceinline__ float smExp(float z, float m) {
#pragma clang fp contract(off)
    return m == -INFINITY ? 0.0f : expf(z - m);
}

// O = acc / s as the contract defines it
__device__ __forceinline__ float attnDiv(float acc, float s, bool dead) {
#pragma clang fp contract(off)
    return dead ? 0.0f : acc / s;
}

}  // namespace bsmr
