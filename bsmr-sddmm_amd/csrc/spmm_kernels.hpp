// Gather-and-accumulate kernels of the SDDMM backward (csrc/backward_capi.hpp, bsmr_spmm / bsmr_sddmm_backward).
//
// For destination d with list L(d):  Y[d,:] = sum_{t in L(d)} v[e(t)] * X[s(t),:]
//   transpose 0: lists = CSR rows,    e(t) = t,             s(t) = col_indices[t]   (X: N x K, Y: M x K)
//   transpose 1: lists = CSC columns, e(t) = csc_to_csr[t], s(t) = csc_rows[t]      (X: M x K, Y: N x K)
//
// A work item is one list or one chunk of at most BSMR_BACKWARD_CHUNK entries of a long list.  K is cut into slices of
// W floats (the widest of 256, 128, 64, 32 that divides K); a unit = (item, slice) belongs to a group of W / V lanes that
// each hold V contiguous floats of the slice: W = 256 -> float4 x 64 lanes, 128 -> float2 x 64 lanes, 64 -> float4 x 16
// lanes (4 units per wave), 32 -> float4 x 8 lanes (8 units per wave).  One wave instruction moves one 1-KiB / 512-B
// source row (W >= 128) or the slices of 4 / 8 different items.  A unit's sum is never split across lanes: each lane runs
// the sequential fp32 fma chain over the list in list order, 4 source rows in flight.  The (s, v) pairs of a list are
// loaded one per lane, G at a time, and broadcast (v_readlane for 64-lane groups, ds_bpermute for narrower ones).
//
// An item of a split list writes its partial row to the workspace; spmmReduce then adds each destination's partials in
// chunk order.  No atomics: every output element has exactly one writer, and its value does not depend on the schedule.
// All row and output addresses are formed in 64 bits (N * K * 4 passes 4 GiB at reddit scale, batches multiply it).
//
// spmmGather16 is the same kernel over a 16-bit X (fp16 or bf16 rows, the copies convertOperands makes): half the
// gathered bytes, every element widened to fp32 - exactly - before the same fma chain, so the result is the fp32 contract
// on (v, round(X)) bit for bit, whichever lane holds which element.
//
// 16-bit outputs (bsmr_spmm_16, bsmr_sddmm_backward_16): spmmGather16 with YT = uint16_t and spmmReduce16 are the same
// gather and the same reduction; only the one store of a finished destination row differs - it rounds the fp32 sums to
// the format of X (bwNarrow: the casts of packLowp) and writes 2 bytes per element.  Chunk partials stay fp32 in the
// workspace, so every output element is rounded exactly once.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sddmm_kernels.hpp"   // u32x4; convertOperands (packLowp), the pass that rounds X

namespace bsmr {

constexpr uint32_t kBwDirect = 0xFFFFFFFFu;   // BwItem.slot: the item owns its whole list and writes Y[dest]

struct BwItem {
    uint32_t dest;    // destination row of Y
    uint32_t begin;   // [begin, end): positions in the direction's list array (CSR index or CSC position)
    uint32_t end;
    uint32_t slot;    // workspace row of this chunk's partial sum, or kBwDirect
};

struct BwSplit {      // a destination whose list was cut into numSlots chunks (partials at firstSlot ...)
    uint32_t dest;
    uint32_t firstSlot;
    uint32_t numSlots;
    uint32_t pad;
};

template <int V> struct BwVec;
template <> struct BwVec<2> {
    using T = float2;
    static __device__ __forceinline__ T zero() { return make_float2(0.f, 0.f); }
    static __device__ __forceinline__ T fma(float w, T x, T a) { return make_float2(fmaf(w, x.x, a.x), fmaf(w, x.y, a.y)); }
};
template <> struct BwVec<4> {
    using T = float4;
    static __device__ __forceinline__ T zero() { return make_float4(0.f, 0.f, 0.f, 0.f); }
    static __device__ __forceinline__ T fma(float w, T x, T a) {
        return make_float4(fmaf(w, x.x, a.x), fmaf(w, x.y, a.y), fmaf(w, x.z, a.z), fmaf(w, x.w, a.w));
    }
};

template <int G>
__device__ __forceinline__ uint32_t bwBroadcast(uint32_t x, uint32_t groupBase, uint32_t j) {
    if constexpr (G == 64) return __builtin_amdgcn_readlane(x, j);   // j is wave-uniform: the whole wave owns one unit
    else return (uint32_t)__shfl((int)x, (int)(groupBase + j), 64);
}

// Slice width W (floats): V floats per lane, G = W / V lanes per unit.  MAP: v is read through map[t] (transpose 1
// with dP read in place); without it v[t].
template <int W, bool MAP>
__global__ void __launch_bounds__(256)
spmmGather(const BwItem* __restrict__ items, uint32_t numItems, uint32_t numSlices, const uint32_t* __restrict__ src,
           const uint32_t* __restrict__ map, const float* __restrict__ v, const float* __restrict__ X,
           float* __restrict__ Y, float* __restrict__ partial, uint32_t K, uint64_t vBatch, uint64_t xBatch,
           uint64_t yBatch, uint64_t pBatch) {
    constexpr int V = W == 128 ? 2 : 4;
    constexpr int G = W / V;
    constexpr int UPW = 64 / G;   // units per wave
    using Vec = BwVec<V>;
    using T = typename Vec::T;
    const uint32_t lane = threadIdx.x & 63u, gl = lane % G, groupBase = lane - gl;
    const uint64_t unit = ((uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6)) * UPW + lane / G;
    if (unit >= (uint64_t)numItems * numSlices) return;   // whole groups leave; a group only reads its own lanes
    const uint32_t it = (uint32_t)(unit / numSlices), slice = (uint32_t)(unit % numSlices);
    const BwItem item = items[it];
    const uint64_t b = blockIdx.y;
    const float* xs = X + b * xBatch + (uint64_t)slice * W + (uint64_t)gl * V;
    const float* vb = v + b * vBatch;
    T acc = Vec::zero();
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
            acc = Vec::fma(w0, x0, acc);
            acc = Vec::fma(w1, x1, acc);
            acc = Vec::fma(w2, x2, acc);
            acc = Vec::fma(w3, x3, acc);
        }
        for (; j < n; ++j) {
            const uint32_t sj = bwBroadcast<G>(s, groupBase, j);
            const float wj = __uint_as_float(bwBroadcast<G>(w, groupBase, j));
            acc = Vec::fma(wj, *reinterpret_cast<const T*>(xs + (uint64_t)sj * K), acc);
        }
    }
    float* dst = item.slot == kBwDirect ? Y + b * yBatch + (uint64_t)item.dest * K
                                        : partial + b * pBatch + (uint64_t)item.slot * K;
    *reinterpret_cast<T*>(dst + (uint64_t)slice * W + (uint64_t)gl * V) = acc;
}

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

template <int MODE, int VE>
__device__ __forceinline__ void bwFma16(float w, const typename BwWords<VE>::T& x, float (&acc)[VE]) {
#pragma unroll
    for (int i = 0; i < VE / 2; ++i) {
        float lo, hi;
        bwWiden<MODE>(x[i], lo, hi);
        acc[2 * i] = fmaf(w, lo, acc[2 * i]);
        acc[2 * i + 1] = fmaf(w, hi, acc[2 * i + 1]);
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

// spmmGather over 16-bit source rows.  W: slice width in elements, as spmmGather; VE: elements per lane (8 = 16-byte
// loads, 4 = 8-byte loads), G = W / VE lanes per unit, 64 / G units per wave.  A lane's load starts VE * 2 bytes into a
// slice that starts W * 2 bytes into a row of K * 2 bytes (K a multiple of W, X 16-byte aligned): naturally aligned, and
// the G loads of a unit cover one slice of one row.  v, the accumulators, the partials and Y are fp32.
// YT = uint16_t: Y holds MODE's 16-bit format too; an item that owns its whole list rounds its sums and stores VE * 2
// bytes per lane (8 or 16, aligned like the loads), a chunk of a split list still writes its fp32 partial.
template <int W, int VE, bool MAP, int MODE, typename YT = float>
__global__ void __launch_bounds__(256)
spmmGather16(const BwItem* __restrict__ items, uint32_t numItems, uint32_t numSlices, const uint32_t* __restrict__ src,
             const uint32_t* __restrict__ map, const float* __restrict__ v, const uint16_t* __restrict__ X,
             YT* __restrict__ Y, float* __restrict__ partial, uint32_t K, uint64_t vBatch, uint64_t xBatch,
             uint64_t yBatch, uint64_t pBatch) {
    constexpr int G = W / VE;
    constexpr int UPW = 64 / G;   // units per wave
    static_assert(G >= 4 && G <= 64 && (VE == 4 || VE == 8), "lane layout");
    using T = typename BwWords<VE>::T;
    const uint32_t lane = threadIdx.x & 63u, gl = lane % G, groupBase = lane - gl;
    const uint64_t unit = ((uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6)) * UPW + lane / G;
    if (unit >= (uint64_t)numItems * numSlices) return;   // whole groups leave; a group only reads its own lanes
    const uint32_t it = (uint32_t)(unit / numSlices), slice = (uint32_t)(unit % numSlices);
    const BwItem item = items[it];
    const uint64_t b = blockIdx.y;
    const uint16_t* xs = X + b * xBatch + (uint64_t)slice * W + (uint64_t)gl * VE;
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
            bwFma16<MODE, VE>(w0, x0, acc);
            bwFma16<MODE, VE>(w1, x1, acc);
            bwFma16<MODE, VE>(w2, x2, acc);
            bwFma16<MODE, VE>(w3, x3, acc);
        }
        for (; j < n; ++j) {
            const uint32_t sj = bwBroadcast<G>(s, groupBase, j);
            const float wj = __uint_as_float(bwBroadcast<G>(w, groupBase, j));
            bwFma16<MODE, VE>(wj, *reinterpret_cast<const T*>(xs + (uint64_t)sj * K), acc);
        }
    }
    if constexpr (sizeof(YT) == 2) {
        const uint64_t col = (uint64_t)slice * W + (uint64_t)gl * VE;
        if (item.slot == kBwDirect) {   // the one store of a finished row
            T o;
#pragma unroll
            for (int i = 0; i < VE / 2; ++i) o[i] = bwNarrow<MODE>(acc[2 * i], acc[2 * i + 1]);
            *reinterpret_cast<T*>(Y + b * yBatch + (uint64_t)item.dest * K + col) = o;
        } else {
            float* dst = partial + b * pBatch + (uint64_t)item.slot * K + col;
#pragma unroll
            for (int i = 0; i < VE; i += 4)
                *reinterpret_cast<float4*>(dst + i) = make_float4(acc[i], acc[i + 1], acc[i + 2], acc[i + 3]);
        }
    } else {
        float* dst = (item.slot == kBwDirect ? Y + b * yBatch + (uint64_t)item.dest * K
                                             : partial + b * pBatch + (uint64_t)item.slot * K) +
                     (uint64_t)slice * W + (uint64_t)gl * VE;
#pragma unroll
        for (int i = 0; i < VE; i += 4)
            *reinterpret_cast<float4*>(dst + i) = make_float4(acc[i], acc[i + 1], acc[i + 2], acc[i + 3]);
    }
}

// Y[dest] = partial[firstSlot] + partial[firstSlot + 1] + ... in chunk order; one thread per 4 floats of a split row.
__global__ void __launch_bounds__(256)
spmmReduce(const BwSplit* __restrict__ splits, uint32_t numSplits, const float* __restrict__ partial,
           float* __restrict__ Y, uint32_t K, uint64_t yBatch, uint64_t pBatch) {
    const uint32_t q = K / 4u;
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= (uint64_t)numSplits * q) return;
    const BwSplit sp = splits[i / q];
    const uint64_t c = (i % q) * 4u;
    const float* p = partial + blockIdx.y * pBatch + (uint64_t)sp.firstSlot * K + c;
    float4 acc = *reinterpret_cast<const float4*>(p);
    for (uint32_t k = 1; k < sp.numSlots; ++k) {
        const float4 x = *reinterpret_cast<const float4*>(p + (uint64_t)k * K);
        acc.x += x.x;
        acc.y += x.y;
        acc.z += x.z;
        acc.w += x.w;
    }
    *reinterpret_cast<float4*>(Y + blockIdx.y * yBatch + (uint64_t)sp.dest * K + c) = acc;
}

// spmmReduce for a 16-bit Y: the same fp32 sum in chunk order, rounded once to MODE's format; 8 bytes per thread.
template <int MODE>
__global__ void __launch_bounds__(256)
spmmReduce16(const BwSplit* __restrict__ splits, uint32_t numSplits, const float* __restrict__ partial,
             uint16_t* __restrict__ Y, uint32_t K, uint64_t yBatch, uint64_t pBatch) {
    const uint32_t q = K / 4u;
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= (uint64_t)numSplits * q) return;
    const BwSplit sp = splits[i / q];
    const uint64_t c = (i % q) * 4u;
    const float* p = partial + blockIdx.y * pBatch + (uint64_t)sp.firstSlot * K + c;
    float4 acc = *reinterpret_cast<const float4*>(p);
    for (uint32_t k = 1; k < sp.numSlots; ++k) {
        const float4 x = *reinterpret_cast<const float4*>(p + (uint64_t)k * K);
        acc.x += x.x;
        acc.y += x.y;
        acc.z += x.z;
        acc.w += x.w;
    }
    u32x2 o;
    o[0] = bwNarrow<MODE>(acc.x, acc.y);
    o[1] = bwNarrow<MODE>(acc.z, acc.w);
    *reinterpret_cast<u32x2*>(Y + blockIdx.y * yBatch + (uint64_t)sp.dest * K + c) = o;
}

// vT[b][t] = v[b][map[t]]: the values in CSC order, once per call (the alternative to reading them through map).
__global__ void __launch_bounds__(256)
spmmPermute(const uint32_t* __restrict__ map, uint32_t nnz, const float* __restrict__ v, float* __restrict__ vT) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= nnz) return;
    const uint64_t b = (uint64_t)blockIdx.y * nnz;
    vT[b + t] = v[b + map[t]];
}

}  // namespace bsmr
