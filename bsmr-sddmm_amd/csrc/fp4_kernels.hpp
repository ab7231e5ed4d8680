// MXFP4 keys and values (csrc/fp4_capi.hpp; include/bsmr_hip.h "MXFP4 keys and values"): the column-side
// operand of the SDDMM (B / Kt), of the SpMM (X / V) and of the fused attention (V) as OCP e2m1 codes, two per byte, with
// one E8M0 scale byte per 32 consecutive elements of a row (E[b][rows][K / 32], as for MXFP8).
//
// A code is 4 bits: bit 3 the sign, bits 2:0 the magnitude 0, 0.5, 1, 1.5, 2, 3, 4, 6 (no infinity, no NaN; code 8 is -0).
// Element 2i of a row is the low nibble of byte i, element 2i + 1 the high nibble (torch.float4_e2m1fn_x2).  Every value
// times a power of two is exact in fp32, so dq = widen(code) * 2^(e - 127) is one exact fp32 multiplication for every scale
// code up to 254 (subnormal products kept, +-inf from 253 on for the large magnitudes, NaN for 255), made in front of the
// fma chain exactly as the MX = true kernels of csrc/fp8_kernels.hpp make it.  bwWiden4 is the one place a nibble becomes
// a number.
//
//   widenFp4Mx    e2m1 + scales -> MODE's 16-bit format, the pass in front of the forward's 16-bit kernels (bsmr_sddmm_b4_mx)
//   spmmGather4   spmmGather8<MX = true> over half-byte source elements: the same BwItem lists and chunk table, one lane
//                 owns an output element's whole fma chain from +0 in list order, 4 source rows in flight, one scale byte
//                 per source row and lane, fp32 chunk partials in the workspace (spmmReduce16 adds and rounds them)
//   attnGather4   attnGather8<MX = true> with the same substitution; attnRowMax and attnReduce are reused as they are
//
// Lane layout: VE source elements per lane - 32 (one 16-byte load) for the slice widths 256 and 128, 16 (one 8-byte load)
// for 64, 8 (one 4-byte load) for 32 - so G = W / VE = 8, 4, 4, 4 lanes per unit and 8, 16, 16, 16 units per wave.  VE <=
// 32 and a lane starts at a multiple of VE elements, so its elements lie in one block of 32: one scale byte per source
// row, at E + s * (K / 32) + col / 32.  No sum is split across lanes: the layout cannot change a bit.  A lane's load starts
// VE / 2 bytes into a slice that starts W / 2 bytes into a row of K / 2 bytes (K a multiple of 32, X 16-byte aligned):
// naturally aligned.  Row addresses s * (K / 2) and the batch stride rows * K / 2 are bytes, formed in 64 bits.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fp8_kernels.hpp"   // bwScaleMx, bwScaleByte, bwStoreNarrow, bwStorePartial; bwBroadcast, attnDiv, smExp behind it

namespace bsmr {

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

// The words one lane loads: VE source elements (8 -> one word, 16 -> u32x2, 32 -> u32x4)
template <int VE> struct BwNibbles;
template <> struct BwNibbles<8> { using T = uint32_t; };
template <> struct BwNibbles<16> { using T = u32x2; };
template <> struct BwNibbles<32> { using T = u32x4; };

template <int VE>
__device__ __forceinline__ uint32_t bwWord4(const typename BwNibbles<VE>::T& x, int i) {
    if constexpr (VE == 8) return x;
    else return x[i];
}

// one source row's term of a lane on dq = widen(code) * sc: the element is dequantised by one fp32 multiplication, then
// enters the chain
template <int VE>
__device__ __forceinline__ void bwFma4Mx(float w, const typename BwNibbles<VE>::T& x, float sc, float (&acc)[VE]) {
#pragma unroll
    for (int i = 0; i < VE / 8; ++i) {
        float e[8];
        bwWiden4(bwWord4<VE>(x, i), e);
#pragma unroll
        for (int k = 0; k < 8; ++k) acc[8 * i + k] = fmaf(w, e[k] * sc, acc[8 * i + k]);
    }
}

// out[i] = narrow(widen(code i) * 2^(scales[i / 32] - 127)): widenFp8Mx over nibbles.  Grid-stride over blocks of 32
// elements: one 16-byte load, one scale byte and four 16-byte stores per lane and step.  count is a multiple of 32, so
// there is no tail.  Offsets are 64-bit.
template <int MODE>
__global__ void __launch_bounds__(256)
widenFp4Mx(const uint8_t* __restrict__ in, const uint8_t* __restrict__ scales, uint16_t* __restrict__ out, uint64_t count) {
    const uint64_t n32 = count / 32u, stride = (uint64_t)gridDim.x * 256u;
    for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < n32; i += stride) {
        const u32x4 w = reinterpret_cast<const u32x4*>(in)[i];
        const float sc = bwScaleMx(scales[i]);
        float x[32];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            float e[8];
            bwWiden4(w[c], e);
#pragma unroll
            for (int k = 0; k < 8; ++k) x[8 * c + k] = e[k] * sc;
        }
        bwStoreNarrow<MODE, 32>(out + i * 32u, x);
    }
}

// W: slice width in elements; VE: source elements per lane (VE / 2 bytes); G = W / VE lanes per unit, 64 / G units per
// wave.  MAP: v is read through map[t].  v, the accumulators and the partials are fp32; Y holds MODE's 16-bit format: an
// item that owns its whole list rounds its sums and stores them, a chunk of a split list writes its fp32 partial.
// The gather runs on dq(X, E): K, yBatch and pBatch are elements, xBatch is bytes (rows * K / 2), eBatch bytes (rows * K / 32).
template <int W, int VE, bool MAP, int MODE>
__global__ void __launch_bounds__(256)
spmmGather4(const BwItem* __restrict__ items, uint32_t numItems, uint32_t numSlices, const uint32_t* __restrict__ src,
            const uint32_t* __restrict__ map, const float* __restrict__ v, const uint8_t* __restrict__ X,
            uint16_t* __restrict__ Y, float* __restrict__ partial, uint32_t K, uint64_t vBatch, uint64_t xBatch,
            uint64_t yBatch, uint64_t pBatch, const uint8_t* __restrict__ E, uint64_t eBatch) {
    constexpr int G = W / VE;
    constexpr int UPW = 64 / G;   // units per wave
    static_assert(G >= 4 && G <= 64 && (VE == 8 || VE == 16 || VE == 32), "lane layout");
    using T = typename BwNibbles<VE>::T;
    const uint32_t lane = threadIdx.x & 63u, gl = lane % G, groupBase = lane - gl;
    const uint64_t unit = ((uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6)) * UPW + lane / G;
    if (unit >= (uint64_t)numItems * numSlices) return;   // whole groups leave; a group only reads its own lanes
    const uint32_t it = (uint32_t)(unit / numSlices), slice = (uint32_t)(unit % numSlices);
    const BwItem item = items[it];
    const uint64_t b = blockIdx.y;
    const uint64_t col = (uint64_t)slice * W + (uint64_t)gl * VE;   // in elements
    const uint8_t* xs = X + b * xBatch + col / 2u;
    const uint8_t* es = E + b * eBatch + col / 32u;
    const uint32_t KH = K / 2u, KB = K / 32u;   // bytes per row of X, of E
    const float* vb = v + b * vBatch;
    float acc[VE];
#pragma unroll
    for (int i = 0; i < VE; ++i) acc[i] = 0.f;
    for (uint32_t t0 = item.begin; t0 < item.end; t0 += G) {
        const uint32_t n = min((uint32_t)G, item.end - t0);
        uint32_t s = 0, w = 0;
        if (gl < n) {
            const uint32_t t = t0 + gl;
            s = src[t];
            w = __float_as_uint(vb[MAP ? map[t] : t]);
        }
        uint32_t j = 0;
        for (; j + 4 <= n; j += 4) {
            const uint32_t s0 = bwBroadcast<G>(s, groupBase, j), s1 = bwBroadcast<G>(s, groupBase, j + 1);
            const uint32_t s2 = bwBroadcast<G>(s, groupBase, j + 2), s3 = bwBroadcast<G>(s, groupBase, j + 3);
            const float w0 = __uint_as_float(bwBroadcast<G>(w, groupBase, j));
            const float w1 = __uint_as_float(bwBroadcast<G>(w, groupBase, j + 1));
            const float w2 = __uint_as_float(bwBroadcast<G>(w, groupBase, j + 2));
            const float w3 = __uint_as_float(bwBroadcast<G>(w, groupBase, j + 3));
            const T x0 = *reinterpret_cast<const T*>(xs + (uint64_t)s0 * KH);
            const T x1 = *reinterpret_cast<const T*>(xs + (uint64_t)s1 * KH);
            const T x2 = *reinterpret_cast<const T*>(xs + (uint64_t)s2 * KH);
            const T x3 = *reinterpret_cast<const T*>(xs + (uint64_t)s3 * KH);
            const uint32_t e0 = bwScaleByte<true>(es, s0, KB), e1 = bwScaleByte<true>(es, s1, KB);
            const uint32_t e2 = bwScaleByte<true>(es, s2, KB), e3 = bwScaleByte<true>(es, s3, KB);
            bwFma4Mx<VE>(w0, x0, bwScaleMx(e0), acc);
            bwFma4Mx<VE>(w1, x1, bwScaleMx(e1), acc);
            bwFma4Mx<VE>(w2, x2, bwScaleMx(e2), acc);
            bwFma4Mx<VE>(w3, x3, bwScaleMx(e3), acc);
        }
        for (; j < n; ++j) {
            const uint32_t sj = bwBroadcast<G>(s, groupBase, j);
            const float wj = __uint_as_float(bwBroadcast<G>(w, groupBase, j));
            bwFma4Mx<VE>(wj, *reinterpret_cast<const T*>(xs + (uint64_t)sj * KH), bwScaleMx(bwScaleByte<true>(es, sj, KB)), acc);
        }
    }
    if (item.slot == kBwDirect)   // the one store of a finished row
        bwStoreNarrow<MODE, VE>(Y + b * yBatch + (uint64_t)item.dest * K + col, acc);
    else
        bwStorePartial<VE>(partial + b * pBatch + (uint64_t)item.slot * K + col, acc);
}

// attnGather8<MX = true> over e2m1 rows of V, O in MODE's 16-bit format: a direct item rounds its quotients once and
// stores them, a chunk item writes its fp32 partial row and partial sum.  The sum of the weights does not see the scales.
// xBatch is bytes (N * K / 2), eBatch bytes (N * K / 32).
template <int W, int VE, int MODE>
__global__ void __launch_bounds__(256)
attnGather4(const BwItem* __restrict__ items, uint32_t numItems, uint32_t numSlices, const uint32_t* __restrict__ src,
            float scale, const float* __restrict__ p, const float* __restrict__ m, const uint8_t* __restrict__ X,
            uint16_t* __restrict__ O, float* __restrict__ sOut, float* __restrict__ partial, float* __restrict__ sPart,
            uint32_t K, uint32_t M, uint32_t numSlots, uint64_t nnz, uint64_t xBatch, const uint8_t* __restrict__ E,
            uint64_t eBatch) {
#pragma clang fp contract(off)
    constexpr int G = W / VE;
    constexpr int UPW = 64 / G;   // units per wave
    static_assert(G >= 4 && G <= 64 && (VE == 8 || VE == 16 || VE == 32), "lane layout");
    using T = typename BwNibbles<VE>::T;
    const uint32_t lane = threadIdx.x & 63u, gl = lane % G, groupBase = lane - gl;
    const uint64_t unit = ((uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6)) * UPW + lane / G;
    if (unit >= (uint64_t)numItems * numSlices) return;   // whole groups leave; a group only reads its own lanes
    const uint32_t it = (uint32_t)(unit / numSlices), slice = (uint32_t)(unit % numSlices);
    const BwItem item = items[it];
    const uint64_t b = blockIdx.y;
    const uint64_t col = (uint64_t)slice * W + (uint64_t)gl * VE;   // in elements
    const uint8_t* xs = X + b * xBatch + col / 2u;
    const uint8_t* es = E + b * eBatch + col / 32u;
    const uint32_t KH = K / 2u, KB = K / 32u;   // bytes per row of V, of E
    const float* pb = p + b * nnz;
    const float mr = m[b * M + item.dest];
    float acc[VE];
#pragma unroll
    for (int i = 0; i < VE; ++i) acc[i] = 0.f;
    float sum = 0.0f;
    for (uint32_t t0 = item.begin; t0 < item.end; t0 += G) {
        const uint32_t n = min((uint32_t)G, item.end - t0);
        uint32_t s = 0, w = 0;
        if (gl < n) {
            const uint32_t t = t0 + gl;
            s = src[t];
            w = __float_as_uint(smExp(scale * pb[t], mr));
        }
        uint32_t j = 0;
        for (; j + 4 <= n; j += 4) {
            const uint32_t s0 = bwBroadcast<G>(s, groupBase, j), s1 = bwBroadcast<G>(s, groupBase, j + 1);
            const uint32_t s2 = bwBroadcast<G>(s, groupBase, j + 2), s3 = bwBroadcast<G>(s, groupBase, j + 3);
            const float w0 = __uint_as_float(bwBroadcast<G>(w, groupBase, j));
            const float w1 = __uint_as_float(bwBroadcast<G>(w, groupBase, j + 1));
            const float w2 = __uint_as_float(bwBroadcast<G>(w, groupBase, j + 2));
            const float w3 = __uint_as_float(bwBroadcast<G>(w, groupBase, j + 3));
            const T x0 = *reinterpret_cast<const T*>(xs + (uint64_t)s0 * KH);
            const T x1 = *reinterpret_cast<const T*>(xs + (uint64_t)s1 * KH);
            const T x2 = *reinterpret_cast<const T*>(xs + (uint64_t)s2 * KH);
            const T x3 = *reinterpret_cast<const T*>(xs + (uint64_t)s3 * KH);
            const uint32_t e0 = bwScaleByte<true>(es, s0, KB), e1 = bwScaleByte<true>(es, s1, KB);
            const uint32_t e2 = bwScaleByte<true>(es, s2, KB), e3 = bwScaleByte<true>(es, s3, KB);
            sum = sum + w0;
            sum = sum + w1;
            sum = sum + w2;
            sum = sum + w3;
            bwFma4Mx<VE>(w0, x0, bwScaleMx(e0), acc);
            bwFma4Mx<VE>(w1, x1, bwScaleMx(e1), acc);
            bwFma4Mx<VE>(w2, x2, bwScaleMx(e2), acc);
            bwFma4Mx<VE>(w3, x3, bwScaleMx(e3), acc);
        }
        for (; j < n; ++j) {
            const uint32_t sj = bwBroadcast<G>(s, groupBase, j);
            const float wj = __uint_as_float(bwBroadcast<G>(w, groupBase, j));
            sum = sum + wj;
            bwFma4Mx<VE>(wj, *reinterpret_cast<const T*>(xs + (uint64_t)sj * KH), bwScaleMx(bwScaleByte<true>(es, sj, KB)), acc);
        }
    }
    if (item.slot == kBwDirect) {   // the one store of a finished row
        const bool dead = mr == -INFINITY;
#pragma unroll
        for (int i = 0; i < VE; ++i) acc[i] = attnDiv(acc[i], sum, dead);
        bwStoreNarrow<MODE, VE>(O + (b * M + item.dest) * K + col, acc);
        if (col == 0) sOut[b * M + item.dest] = sum;
    } else {
        bwStorePartial<VE>(partial + (b * numSlots + item.slot) * K + col, acc);
        if (col == 0) sPart[b * numSlots + item.slot] = sum;
    }
}

}  // namespace bsmr
