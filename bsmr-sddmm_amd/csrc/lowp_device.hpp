// Device helpers of the 16-bit operand formats (MODE 0: fp16, MODE 1: bf16): the vector types, rounding fp32 to a format
// (packLowp, bwNarrow), widening it back exactly (bwWiden) and the dot product of two 16-byte chunks (dot2, ResidueLowp).
// Helpers only - no kernel is defined here - so any translation unit may include it (DESIGN.md 18 departure (4)).  The
// kernels that use them: csrc/sddmm_kernels.hpp, csrc/spmm_kernels.hpp and the one-pass attention units.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace bsmr {

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x3 __attribute__((ext_vector_type(3)));

template <int MODE>
__device__ __forceinline__ u32x4 packLowp(const f32x4& lo, const f32x4& hi) {
    if constexpr (MODE == 0) {
        f16x8 o;
        o[0] = (_Float16)lo[0]; o[1] = (_Float16)lo[1]; o[2] = (_Float16)lo[2]; o[3] = (_Float16)lo[3];
        o[4] = (_Float16)hi[0]; o[5] = (_Float16)hi[1]; o[6] = (_Float16)hi[2]; o[7] = (_Float16)hi[3];
        return __builtin_bit_cast(u32x4, o);
    } else {
        bf16x8 o;
        o[0] = (__bf16)lo[0]; o[1] = (__bf16)lo[1]; o[2] = (__bf16)lo[2]; o[3] = (__bf16)lo[3];
        o[4] = (__bf16)hi[0]; o[5] = (__bf16)hi[1]; o[6] = (__bf16)hi[2]; o[7] = (__bf16)hi[3];
        return __builtin_bit_cast(u32x4, o);
    }
}

template <int MODE>
__device__ __forceinline__ float dot2(uint32_t a, uint32_t b, float acc) {
    if constexpr (MODE == 0) {
        typedef _Float16 h2 __attribute__((ext_vector_type(2)));
        return __builtin_amdgcn_fdot2(__builtin_bit_cast(h2, a), __builtin_bit_cast(h2, b), acc, false);
    } else {
        typedef __bf16 b2 __attribute__((ext_vector_type(2)));
        return __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(b2, a), __builtin_bit_cast(b2, b), acc, false);
    }
}

// One step of a 16 x 16 product over 32 k on v_mfma_f32_16x16x32_f16 / _bf16: lane l holds A[l & 15][8 (l >> 4) ... + 7] in
// a, B[8 (l >> 4) ... + 7][l & 15] in b and C[4 (l >> 4) + i][l & 15] in c[i].  The one-pass attention units on the MFMA.
template <int MODE>
__device__ __forceinline__ f32x4 mfmaLowp(const u32x4 a, const u32x4 b, const f32x4 c) {
    if constexpr (MODE == 0)
        return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
    else
        return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}

// The element policy of the fp16 / bf16 operand copies (csrc/sddmm_kernels.hpp, "Sparse residue"): 8 elements per
// 16-byte chunk through v_dot2c_f32_{f16,bf16} (products exact, fp32 accumulation), four steps in ascending k.
template <int MODE>
struct ResidueLowp {
    typedef uint16_t elem;
    typedef u32x4 chunk;
    typedef uint8_t unit;
    static constexpr uint32_t kPerChunk = 8;
    static __device__ __forceinline__ float dot(const chunk& a, const chunk& b, float acc) {
        acc = dot2<MODE>(a[0], b[0], acc);
        acc = dot2<MODE>(a[1], b[1], acc);
        acc = dot2<MODE>(a[2], b[2], acc);
        acc = dot2<MODE>(a[3], b[3], acc);
        return acc;
    }
    static __device__ __forceinline__ chunk round(const f32x4& lo, const f32x4& hi) { return packLowp<MODE>(lo, hi); }
};

// The 16-bit words one lane loads (VE elements: 8 -> 16 bytes, 4 -> 8 bytes) and their exact widening to fp32.
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
template <int VE> struct BwWords;
template <> struct BwWords<4> { using T = u32x2; };
template <> struct BwWords<8> { using T = u32x4; };

// MODE 0: two fp16 (v_cvt_f32_f16 keeps fp16 subnormals, inf and NaN); MODE 1: two bf16 (the upper half of an fp32).
// Element 2i is the low half of word i.
template <int MODE>
__device__ __forceinline__ void bwWiden(uint32_t pair, float& lo, float& hi) {
    if constexpr (MODE == 0) {
        typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
        const f16x2 h = __builtin_bit_cast(f16x2, pair);
        lo = (float)h[0];
        hi = (float)h[1];
    } else {
        lo = __uint_as_float(pair << 16);
        hi = __uint_as_float(pair & 0xFFFF0000u);
    }
}

// Two fp32 sums rounded to MODE's format (round to nearest even, fp16 subnormals kept, +-inf beyond the range, NaN stays
// NaN: the casts of packLowp), element 2i in the low half of word i - the inverse of bwWiden.
template <int MODE>
__device__ __forceinline__ uint32_t bwNarrow(float lo, float hi) {
    if constexpr (MODE == 0) {
        typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
        f16x2 o;
        o[0] = (_Float16)lo;
        o[1] = (_Float16)hi;
        return __builtin_bit_cast(uint32_t, o);
    } else {
        typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
        bf16x2 o;
        o[0] = (__bf16)lo;
        o[1] = (__bf16)hi;
        return __builtin_bit_cast(uint32_t, o);
    }
}

}  // namespace bsmr
