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
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

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

// vT[b][t] = v[b][map[t]]: the values in CSC order, once per call (the alternative to reading them through map).
__global__ void __launch_bounds__(256)
spmmPermute(const uint32_t* __restrict__ map, uint32_t nnz, const float* __restrict__ v, float* __restrict__ vT) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= nnz) return;
    const uint64_t b = (uint64_t)blockIdx.y * nnz;
    vT[b + t] = v[b + map[t]];
}

}  // namespace bsmr
