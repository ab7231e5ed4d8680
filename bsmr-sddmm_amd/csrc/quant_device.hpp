// Device helpers of the quantised key / value formats (csrc/fp8_kernels.hpp, csrc/fp4_kernels.hpp): the one place an fp8
// byte (bwWiden8), an e2m1 nibble (bwWiden4) or an E8M0 block scale (bwScaleMx) becomes a number.  Helpers only - no kernel
// is defined here - so the one-pass attention unit of the quantised KV cache includes it without the gather kernels.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace bsmr {

// The four codes of a 32-bit word (element i in byte i), widened exactly to fp32.
template <int FMT>
__device__ __forceinline__ void bwWiden8(uint32_t word, float (&x)[4]) {
    typedef float f32x2 __attribute__((ext_vector_type(2)));
    f32x2 lo, hi;
    if constexpr (FMT == 0) {
        lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)word, false);
        hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)word, true);
    } else {
        lo = __builtin_amdgcn_cvt_pk_f32_bf8((int)word, false);
        hi = __builtin_amdgcn_cvt_pk_f32_bf8((int)word, true);
    }
    x[0] = lo[0];
    x[1] = lo[1];
    x[2] = hi[0];
    x[3] = hi[1];
}

// 2^(e - 127) for an E8M0 code, built from bits: 1 .. 254 are the exponent field of a normal, 0 is the subnormal
// 2^-127, 255 a quiet NaN
__device__ __forceinline__ float bwScaleMx(uint32_t e) {
    return __uint_as_float(e == 0u ? 0x00400000u : e == 255u ? 0x7FC00000u : e << 23);
}

// The eight codes of a 32-bit word (element i in nibble i, the low nibble of a byte first), widened exactly to fp32:
// v_cvt_scalef32_pk_f32_fp4 at scale 1.0 turns the two nibbles of one byte into two fp32 (-0 keeps its sign), op_sel
// picks the byte.  The block scale is a separate fp32 multiplication (bwFma4Mx), as for fp8.
__device__ __forceinline__ void bwWiden4(uint32_t word, float (&x)[8]) {
    typedef float f32x2 __attribute__((ext_vector_type(2)));
    const f32x2 b0 = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(word, 1.0f, 0);
    const f32x2 b1 = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(word, 1.0f, 1);
    const f32x2 b2 = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(word, 1.0f, 2);
    const f32x2 b3 = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(word, 1.0f, 3);
    x[0] = b0[0];
    x[1] = b0[1];
    x[2] = b1[0];
    x[3] = b1[1];
    x[4] = b2[0];
    x[5] = b2[1];
    x[6] = b3[0];
    x[7] = b3[1];
}

}  // namespace bsmr
