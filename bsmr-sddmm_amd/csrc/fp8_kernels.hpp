// fp8 keys and values (csrc/fp8_capi.hpp; include/bsmr_hip.h "fp8 keys and values"): the column-side operand
// of the SDDMM (B / Kt), of the SpMM (X / V) and of the fused attention (V) as OCP fp8 bytes - FMT 0: e4m3fn, FMT 1: e5m2.
//
// Every code of both formats is a value of fp16 and of bf16 (3 / 2 mantissa bits, exponents inside both ranges, the
// subnormals of fp8 normal in either), so widening is exact and an fp8 call is, bit for bit, the 16-bit call on the
// widened operand.  bwWiden8 is the one place a code becomes a number: v_cvt_pk_f32_fp8 / _bf8 turn two bytes of a
// register into two fp32 (+-0 keeps its sign, subnormals exact, e5m2 +-inf stays +-inf, every NaN code a NaN).
//
//   widenFp8      fp8 -> MODE's 16-bit format, the pass in front of the forward's 16-bit kernels (bsmr_sddmm_b8)
//   spmmGather8   spmmGather16 over 1-byte source elements with a 16-bit Y: the same BwItem lists and chunk table, one
//                 lane owns an output element's whole fma chain from +0 in list order, 4 source rows in flight, fp32
//                 chunk partials in the workspace (spmmReduce16 adds and rounds them), one rounding per output element
//   attnGather8   attnGather16 with the same substitution; attnRowMax and attnReduce are reused as they are
//
// MX block scales: one E8M0 byte per 32 consecutive elements of a row, E[b][rows][K/32]; code e is
// 2^(e-127), 255 is NaN.  dq = widen(code) * scale is one fp32 multiplication (subnormal products kept, overflow to
// +-inf) in front of the fma chain.  widenFp8Mx and the MX = true instantiations of the gathers are the kernels above
// with that one multiplication (MX = false compiles the scale away, E is then never read), so lists, chunks, rows in
// flight, lane layout, partials and reduce kernels are the same.  A lane's VE bytes lie in one block of 32, so it loads
// one scale byte per source row, at E + s * (K / 32) + col / 32.
//
// Lane layout: VE source bytes per lane - 16 (one 16-byte load) for the slice widths 256 and 128, 8 (one 8-byte load)
// for 64 and 32 - so G = W / VE = 16, 8, 8, 4 lanes per unit and 4, 8, 8, 16 units per wave.  No sum is split across
// lanes: the layout cannot change a bit.  A lane's load starts VE bytes into a slice that starts W bytes into a row of K
// bytes (K a multiple of 32, X 16-byte aligned): naturally aligned.  Row addresses s * K and the batch stride rows * K
// are bytes, formed in 64 bits.  A finished row stores VE 16-bit elements per lane: one or two 16-byte stores.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "attention_kernels.hpp"   // spmm_kernels.hpp: BwItem, BwWords, bwBroadcast, bwNarrow; attnDiv, smExp

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

// The words one lane loads: VE source bytes (8 -> u32x2, 16 -> u32x4)
template <int VE> using BwBytes = typename BwWords<VE / 2>::T;

template <int FMT, int VE>
__device__ __forceinline__ void bwFma8(float w, const BwBytes<VE>& x, float (&acc)[VE]) {
#pragma unroll
    for (int i = 0; i < VE / 4; ++i) {
        float e[4];
        bwWiden8<FMT>(x[i], e);
#pragma unroll
        for (int k = 0; k < 4; ++k) acc[4 * i + k] = fmaf(w, e[k], acc[4 * i + k]);
    }
}

// 2^(e - 127) for an E8M0 code, built from bits: 1 .. 254 are the exponent field of a normal, 0 is the subnormal
// 2^-127, 255 a quiet NaN
__device__ __forceinline__ float bwScaleMx(uint32_t e) {
    return __uint_as_float(e == 0u ? 0x00400000u : e == 255u ? 0x7FC00000u : e << 23);
}

// bwFma8 on dq = widen(code) * sc: the element is dequantised by one fp32 multiplication, then enters the chain
template <int FMT, int VE>
__device__ __forceinline__ void bwFma8Mx(float w, const BwBytes<VE>& x, float sc, float (&acc)[VE]) {
#pragma unroll
    for (int i = 0; i < VE / 4; ++i) {
        float e[4];
        bwWiden8<FMT>(x[i], e);
#pragma unroll
        for (int k = 0; k < 4; ++k) acc[4 * i + k] = fmaf(w, e[k] * sc, acc[4 * i + k]);
    }
}

// the scale code of source row s for a lane whose block column es points at (KB = K / 32 bytes per row)
template <bool MX>
__device__ __forceinline__ uint32_t bwScaleByte(const uint8_t* es, uint32_t s, uint32_t KB) {
    if constexpr (MX) return es[(uint64_t)s * KB];
    else return 0u;
}

// one source row's term of a lane: the row's bytes x, its scale code e (MX)
template <int FMT, int VE, bool MX>
__device__ __forceinline__ void bwRowFma8(float w, const BwBytes<VE>& x, uint32_t e, float (&acc)[VE]) {
    if constexpr (MX) bwFma8Mx<FMT, VE>(w, x, bwScaleMx(e), acc);
    else bwFma8<FMT, VE>(w, x, acc);
}

// VE fp32 sums of a finished row, rounded once to MODE's format: 16 bytes per store
template <int MODE, int VE>
__device__ __forceinline__ void bwStoreNarrow(uint16_t* dst, const float (&acc)[VE]) {
#pragma unroll
    for (int i = 0; i < VE; i += 8) {
        u32x4 o;
#pragma unroll
        for (int k = 0; k < 4; ++k) o[k] = bwNarrow<MODE>(acc[i + 2 * k], acc[i + 2 * k + 1]);
        *reinterpret_cast<u32x4*>(dst + i) = o;
    }
}

template <int VE>
__device__ __forceinline__ void bwStorePartial(float* dst, const float (&acc)[VE]) {
#pragma unroll
    for (int i = 0; i < VE; i += 4)
        *reinterpret_cast<float4*>(dst + i) = make_float4(acc[i], acc[i + 1], acc[i + 2], acc[i + 3]);
}

// out[i] = widen(in[i]) for i < count, in MODE's 16-bit format.  Grid-stride over groups of 16 elements: one 16-byte load
// and two 16-byte stores per lane and step; the last count % 16 elements one per thread.  Offsets are 64-bit.
template <int MODE, int FMT>
__global__ void __launch_bounds__(256)
widenFp8(const uint8_t* __restrict__ in, uint16_t* __restrict__ out, uint64_t count) {
    const uint64_t n16 = count / 16u, stride = (uint64_t)gridDim.x * 256u;
    const uint64_t tid = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    for (uint64_t i = tid; i < n16; i += stride) {
        const u32x4 w = reinterpret_cast<const u32x4*>(in)[i];
        float x[16];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            float e[4];
            bwWiden8<FMT>(w[c], e);
#pragma unroll
            for (int k = 0; k < 4; ++k) x[4 * c + k] = e[k];
        }
        bwStoreNarrow<MODE, 16>(out + i * 16u, x);
    }
    const uint64_t t = n16 * 16u + tid;
    if (t < count) {
        float e[4];
        bwWiden8<FMT>(in[t], e);
        out[t] = (uint16_t)bwNarrow<MODE>(e[0], 0.0f);
    }
}

// out[i] = narrow(widen(in[i]) * 2^(scales[i / 32] - 127)): widenFp8 with one scale byte per group of 16 elements (group
// i lies in block i / 2).  count is a multiple of 32, so there is no tail.
template <int MODE, int FMT>
__global__ void __launch_bounds__(256)
widenFp8Mx(const uint8_t* __restrict__ in, const uint8_t* __restrict__ scales, uint16_t* __restrict__ out, uint64_t count) {
    const uint64_t n16 = count / 16u, stride = (uint64_t)gridDim.x * 256u;
    for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < n16; i += stride) {
        const u32x4 w = reinterpret_cast<const u32x4*>(in)[i];
        const float sc = bwScaleMx(scales[i / 2u]);
        float x[16];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            float e[4];
            bwWiden8<FMT>(w[c], e);
#pragma unroll
            for (int k = 0; k < 4; ++k) x[4 * c + k] = e[k] * sc;
        }
        bwStoreNarrow<MODE, 16>(out + i * 16u, x);
    }
}

// W: slice width in elements; VE: source bytes per lane; G = W / VE lanes per unit, 64 / G units per wave.  MAP: v is
// read through map[t].  v, the accumulators and the partials are fp32; Y holds MODE's 16-bit format: an item that owns
// its whole list rounds its sums and stores them, a chunk of a split list writes its fp32 partial.
// MX: the gather runs on dq(X, E) - every widened element is multiplied by its block's scale, read from E ([b][rows][K / 32]
// bytes, batch stride eBatch).  Without MX (the default: bsmr_spmm_x8) the two last arguments are never read and the
// instantiation is, instruction for instruction, the kernel it was before they existed.
template <int W, int VE, bool MAP, int MODE, int FMT, bool MX = false>
__global__ void __launch_bounds__(256)
spmmGather8(const BwItem* __restrict__ items, uint32_t numItems, uint32_t numSlices, const uint32_t* __restrict__ src,
            const uint32_t* __restrict__ map, const float* __restrict__ v, const uint8_t* __restrict__ X,
            uint16_t* __restrict__ Y, float* __restrict__ partial, uint32_t K, uint64_t vBatch, uint64_t xBatch,
            uint64_t yBatch, uint64_t pBatch, const uint8_t* __restrict__ E, uint64_t eBatch) {
    constexpr int G = W / VE;
    constexpr int UPW = 64 / G;   // units per wave
    static_assert(G >= 4 && G <= 64 && (VE == 8 || VE == 16), "lane layout");
    using T = BwBytes<VE>;
    const uint32_t lane = threadIdx.x & 63u, gl = lane % G, groupBase = lane - gl;
    const uint64_t unit = ((uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6)) * UPW + lane / G;
    if (unit >= (uint64_t)numItems * numSlices) return;   // whole groups leave; a group only reads its own lanes
    const uint32_t it = (uint32_t)(unit / numSlices), slice = (uint32_t)(unit % numSlices);
    const BwItem item = items[it];
    const uint64_t b = blockIdx.y;
    const uint64_t col = (uint64_t)slice * W + (uint64_t)gl * VE;
    const uint8_t* xs = X + b * xBatch + col;
    const uint8_t* es = MX ? E + b * eBatch + col / 32u : nullptr;
    const uint32_t KB = K / 32u;
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
            const T x0 = *reinterpret_cast<const T*>(xs + (uint64_t)s0 * K);
            const T x1 = *reinterpret_cast<const T*>(xs + (uint64_t)s1 * K);
            const T x2 = *reinterpret_cast<const T*>(xs + (uint64_t)s2 * K);
            const T x3 = *reinterpret_cast<const T*>(xs + (uint64_t)s3 * K);
            const uint32_t e0 = bwScaleByte<MX>(es, s0, KB), e1 = bwScaleByte<MX>(es, s1, KB);
            const uint32_t e2 = bwScaleByte<MX>(es, s2, KB), e3 = bwScaleByte<MX>(es, s3, KB);
            bwRowFma8<FMT, VE, MX>(w0, x0, e0, acc);
            bwRowFma8<FMT, VE, MX>(w1, x1, e1, acc);
            bwRowFma8<FMT, VE, MX>(w2, x2, e2, acc);
            bwRowFma8<FMT, VE, MX>(w3, x3, e3, acc);
        }
        for (; j < n; ++j) {
            const uint32_t sj = bwBroadcast<G>(s, groupBase, j);
            const float wj = __uint_as_float(bwBroadcast<G>(w, groupBase, j));
            bwRowFma8<FMT, VE, MX>(wj, *reinterpret_cast<const T*>(xs + (uint64_t)sj * K), bwScaleByte<MX>(es, sj, KB), acc);
        }
    }
    if (item.slot == kBwDirect)   // the one store of a finished row
        bwStoreNarrow<MODE, VE>(Y + b * yBatch + (uint64_t)item.dest * K + col, acc);
    else
        bwStorePartial<VE>(partial + b * pBatch + (uint64_t)item.slot * K + col, acc);
}

// attnGather16 over fp8 rows of V, O in MODE's 16-bit format: a direct item rounds its quotients once and stores them, a
// chunk item writes its fp32 partial row and partial sum.
// MX: on dq(V, E), as in spmmGather8; the sum of the weights does not see the scales.
template <int W, int VE, int MODE, int FMT, bool MX = false>
__global__ void __launch_bounds__(256)
attnGather8(const BwItem* __restrict__ items, uint32_t numItems, uint32_t numSlices, const uint32_t* __restrict__ src,
            float scale, const float* __restrict__ p, const float* __restrict__ m, const uint8_t* __restrict__ X,
            uint16_t* __restrict__ O, float* __restrict__ sOut, float* __restrict__ partial, float* __restrict__ sPart,
            uint32_t K, uint32_t M, uint32_t numSlots, uint64_t nnz, uint64_t xBatch, const uint8_t* __restrict__ E,
            uint64_t eBatch) {
#pragma clang fp contract(off)
    constexpr int G = W / VE;
    constexpr int UPW = 64 / G;   // units per wave
    static_assert(G >= 4 && G <= 64 && (VE == 8 || VE == 16), "lane layout");
    using T = BwBytes<VE>;
    const uint32_t lane = threadIdx.x & 63u, gl = lane % G, groupBase = lane - gl;
    const uint64_t unit = ((uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6)) * UPW + lane / G;
    if (unit >= (uint64_t)numItems * numSlices) return;   // whole groups leave; a group only reads its own lanes
    const uint32_t it = (uint32_t)(unit / numSlices), slice = (uint32_t)(unit % numSlices);
    const BwItem item = items[it];
    const uint64_t b = blockIdx.y;
    const uint64_t col = (uint64_t)slice * W + (uint64_t)gl * VE;
    const uint8_t* xs = X + b * xBatch + col;
    const uint8_t* es = MX ? E + b * eBatch + col / 32u : nullptr;
    const uint32_t KB = K / 32u;
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
            const T x0 = *reinterpret_cast<const T*>(xs + (uint64_t)s0 * K);
            const T x1 = *reinterpret_cast<const T*>(xs + (uint64_t)s1 * K);
            const T x2 = *reinterpret_cast<const T*>(xs + (uint64_t)s2 * K);
            const T x3 = *reinterpret_cast<const T*>(xs + (uint64_t)s3 * K);
            const uint32_t e0 = bwScaleByte<MX>(es, s0, KB), e1 = bwScaleByte<MX>(es, s1, KB);
            const uint32_t e2 = bwScaleByte<MX>(es, s2, KB), e3 = bwScaleByte<MX>(es, s3, KB);
            sum = sum + w0;
            sum = sum + w1;
            sum = sum + w2;
            sum = sum + w3;
            bwRowFma8<FMT, VE, MX>(w0, x0, e0, acc);
            bwRowFma8<FMT, VE, MX>(w1, x1, e1, acc);
            bwRowFma8<FMT, VE, MX>(w2, x2, e2, acc);
            bwRowFma8<FMT, VE, MX>(w3, x3, e3, acc);
        }
        for (; j < n; ++j) {
            const uint32_t sj = bwBroadcast<G>(s, groupBase, j);
            const float wj = __uint_as_float(bwBroadcast<G>(w, groupBase, j));
            sum = sum + wj;
            bwRowFma8<FMT, VE, MX>(wj, *reinterpret_cast<const T*>(xs + (uint64_t)sj * K), bwScaleByte<MX>(es, sj, KB), acc);
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
