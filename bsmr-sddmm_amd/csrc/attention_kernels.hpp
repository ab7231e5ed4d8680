// Fused softmax . V of sparse attention and its backward (csrc/attention_capi.hpp, bsmr_sparse_attention / _backward;
// include/bsmr_hip.h "Fused sparse attention").
//
// Forward, per row r of S with scores p_t in CSR order (every step one IEEE fp32 operation, fp contraction off):
//   z_t = fl(scale p_t);  m = max_t z_t (NaN if any z is NaN);  e_t = expf(fl(z_t - m)) (0 when m = -inf);
//   s = sum_t e_t;  acc_k = sum_t fmaf(e_t, V[c_t, k], .);  O_k = acc_k / s (+0 when m = -inf or the row is empty)
// attnRowMax writes m; attnGather is spmmGather's row direction (same BwItem lists, chunk table, lane layouts,
// broadcasts, 4 source rows in flight) with two additions: the lane that loads entry t turns its score into e_t before
// the broadcast (one expf per entry per unit), and every lane carries one more accumulator, s, fed by the same broadcast
// weights in the same order - the same chain on every lane, so whichever lane stores it stores the same bits.  s and acc
// run in bsmr_spmm's order: a sequential chain from +0 in CSR order; a row longer than BSMR_BACKWARD_CHUNK is the
// handle's chunks, whose fp32 partial rows and partial sums go to the workspace and are added in chunk order by
// attnReduce, which then divides.  An item that owns its whole row divides and stores O and s itself.
// No atomics: every output element has one writer and its value does not depend on the schedule.
//
// Backward, per row:  D = dO_r . O_r;  per entry:  w_t = fl(e_t / s) (e_t recomputed from p_t, m, s; 0 when m = -inf);
//   dP_t = fl(fl(w_t fl(dW_t - D)) scale);  W_t = w_t  (for the transposed SpMM that gives dV)
// attnRowDot fixes D's order: 32 lanes per row, lane l runs the fma chain over k = l, l + 32, ... ascending from +0, the
// 32 partials are added by a butterfly over the offsets 16, 8, 4, 2, 1 (fp32 addition commutes: all lanes end equal).
// attnValuesBackward finds an entry's row as the softmax kernels do: a row of at most BSMR_BACKWARD_CHUNK entries is one
// wave's, a longer one (the handle's row chunk table) one workgroup's.  dP may alias dW: each position is read and
// written by the same thread, so neither is __restrict__.
//
// 16-bit forms: V, O, dO are fp16 / bf16 rows, widened exactly (bwWiden); sums stay fp32; O is rounded once (bwNarrow)
// by the single store of a finished row.  All addresses are formed in 64 bits.
#pragma once

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "softmax_kernels.hpp"   // smWaveMax, smRowMax, smBlockMax, smExp, kSmChunk; spmm_kernels.hpp

namespace bsmr {

// m[b][r] for every row.  Blocks [0, shortBlocks): one wave per row of at most kSmChunk entries, 4 rows per block
// (an empty row: -inf); blocks behind them: one block per row of the chunk table.
__global__ void __launch_bounds__(256)
attnRowMax(const uint32_t* __restrict__ ro, const BwSplit* __restrict__ splits, uint32_t M, uint32_t shortBlocks,
           float scale, const float* __restrict__ P, float* __restrict__ m, uint64_t nnz) {
#pragma clang fp contract(off)
    __shared__ float red[4];
    const uint64_t bM = (uint64_t)blockIdx.y * M;
    if (blockIdx.x >= shortBlocks) {
        const uint32_t row = splits[blockIdx.x - shortBlocks].dest;
        const uint32_t b = ro[row], n = ro[row + 1] - b;
        const uint64_t base = (uint64_t)blockIdx.y * nnz + b;
        float mx = -INFINITY;
        bool nan = false;
        for (uint32_t i = threadIdx.x; i < n; i += 256u) {
            const float z = scale * P[base + i];
            mx = fmaxf(mx, z);
            nan |= z != z;
        }
        mx = smBlockMax(mx, nan, red);
        if (threadIdx.x == 0) m[bM + row] = mx;
        return;
    }
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t r = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (r >= M) return;
    const uint32_t b = ro[r], n = ro[r + 1] - b;
    if (n > kSmChunk) return;   // (the chunk table's rows)
    const uint64_t base = (uint64_t)blockIdx.y * nnz + b;
    float mx = -INFINITY;
    bool nan = false;
    for (uint32_t i = lane; i < n; i += 64u) {
        const float z = scale * P[base + i];
        mx = fmaxf(mx, z);
        nan |= z != z;
    }
    mx = smRowMax(smWaveMax(mx), __any(nan));
    if (lane == 0) m[bM + r] = mx;
}

// O = acc / s as the contract defines it
__device__ __forceinline__ float attnDiv(float acc, float s, bool dead) {
#pragma clang fp contract(off)
    return dead ? 0.0f : acc / s;
}

// Slice width W (floats) and lane layout as spmmGather.  p: the scores [b][nnz]; m: [b][M]; a direct item stores
// O[dest] and s[dest], a chunk item its partial row (partial, [b][numSlots][K]) and partial sum (sPart, [b][numSlots]).
template <int W>
__global__ void __launch_bounds__(256)
attnGather(const BwItem* __restrict__ items, uint32_t numItems, uint32_t numSlices, const uint32_t* __restrict__ src,
           float scale, const float* __restrict__ p, const float* __restrict__ m, const float* __restrict__ X,
           float* __restrict__ O, float* __restrict__ sOut, float* __restrict__ partial, float* __restrict__ sPart,
           uint32_t K, uint32_t M, uint32_t numSlots, uint64_t nnz, uint64_t xBatch) {
#pragma clang fp contract(off)
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
    const float* pb = p + b * nnz;
    const float mr = m[b * M + item.dest];
    T acc = Vec::zero();
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
            sum = sum + w0;
            sum = sum + w1;
            sum = sum + w2;
            sum = sum + w3;
            acc = Vec::fma(w0, x0, acc);
            acc = Vec::fma(w1, x1, acc);
            acc = Vec::fma(w2, x2, acc);
            acc = Vec::fma(w3, x3, acc);
        }
        for (; j < n; ++j) {
            const uint32_t sj = bwBroadcast<G>(s, groupBase, j);
            const float wj = __uint_as_float(bwBroadcast<G>(w, groupBase, j));
            sum = sum + wj;
            acc = Vec::fma(wj, *reinterpret_cast<const T*>(xs + (uint64_t)sj * K), acc);
        }
    }
    const uint64_t col = (uint64_t)slice * W + (uint64_t)gl * V;
    if (item.slot == kBwDirect) {
        const bool dead = mr == -INFINITY;   // (an empty row too: attnRowMax gives it -inf)
        T o;
        o.x = attnDiv(acc.x, sum, dead);
        o.y = attnDiv(acc.y, sum, dead);
        if constexpr (V == 4) {
            o.z = attnDiv(acc.z, sum, dead);
            o.w = attnDiv(acc.w, sum, dead);
        }
        *reinterpret_cast<T*>(O + (b * M + item.dest) * K + col) = o;
        if (col == 0) sOut[b * M + item.dest] = sum;
    } else {
        *reinterpret_cast<T*>(partial + (b * numSlots + item.slot) * K + col) = acc;
        if (col == 0) sPart[b * numSlots + item.slot] = sum;
    }
}

// attnGather over 16-bit rows of V (lane layouts of spmmGather16) with a 16-bit O in the same format: a direct item
// rounds its quotients once and stores VE * 2 bytes per lane, a chunk item writes its fp32 partials.
template <int W, int VE, int MODE>
__global__ void __launch_bounds__(256)
attnGather16(const BwItem* __restrict__ items, uint32_t numItems, uint32_t numSlices, const uint32_t* __restrict__ src,
             float scale, const float* __restrict__ p, const float* __restrict__ m, const uint16_t* __restrict__ X,
             uint16_t* __restrict__ O, float* __restrict__ sOut, float* __restrict__ partial,
             float* __restrict__ sPart, uint32_t K, uint32_t M, uint32_t numSlots, uint64_t nnz, uint64_t xBatch) {
#pragma clang fp contract(off)
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
            sum = sum + w0;
            sum = sum + w1;
            sum = sum + w2;
            sum = sum + w3;
            bwFma16<MODE, VE>(w0, x0, acc);
            bwFma16<MODE, VE>(w1, x1, acc);
            bwFma16<MODE, VE>(w2, x2, acc);
            bwFma16<MODE, VE>(w3, x3, acc);
        }
        for (; j < n; ++j) {
            const uint32_t sj = bwBroadcast<G>(s, groupBase, j);
            const float wj = __uint_as_float(bwBroadcast<G>(w, groupBase, j));
            sum = sum + wj;
            bwFma16<MODE, VE>(wj, *reinterpret_cast<const T*>(xs + (uint64_t)sj * K), acc);
        }
    }
    const uint64_t col = (uint64_t)slice * W + (uint64_t)gl * VE;
    if (item.slot == kBwDirect) {   // the one store of a finished row
        const bool dead = mr == -INFINITY;
        T o;
#pragma unroll
        for (int i = 0; i < VE / 2; ++i)
            o[i] = bwNarrow<MODE>(attnDiv(acc[2 * i], sum, dead), attnDiv(acc[2 * i + 1], sum, dead));
        *reinterpret_cast<T*>(O + (b * M + item.dest) * K + col) = o;
        if (col == 0) sOut[b * M + item.dest] = sum;
    } else {
        float* dst = partial + (b * numSlots + item.slot) * K + col;
#pragma unroll
        for (int i = 0; i < VE; i += 4)
            *reinterpret_cast<float4*>(dst + i) = make_float4(acc[i], acc[i + 1], acc[i + 2], acc[i + 3]);
        if (col == 0) sPart[b * numSlots + item.slot] = sum;
    }
}

// A split row: acc and s partials added in chunk order, then the division; one thread per 4 floats of the row.
// MODE < 0: fp32 O; 0 / 1: O in fp16 / bf16, rounded once.
template <int MODE>
__global__ void __launch_bounds__(256)
attnReduce(const BwSplit* __restrict__ splits, uint32_t numSplits, const float* __restrict__ partial,
           const float* __restrict__ sPart, const float* __restrict__ m, void* __restrict__ Oout,
           float* __restrict__ sOut, uint32_t K, uint32_t M, uint32_t numSlots) {
#pragma clang fp contract(off)
    const uint32_t q = K / 4u;
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= (uint64_t)numSplits * q) return;
    const BwSplit sp = splits[i / q];
    const uint64_t c = (i % q) * 4u;
    const uint64_t b = blockIdx.y;
    const float* pp = partial + (b * numSlots + sp.firstSlot) * K + c;
    const float* ps = sPart + b * numSlots + sp.firstSlot;
    float4 acc = *reinterpret_cast<const float4*>(pp);
    float sum = ps[0];
    for (uint32_t k = 1; k < sp.numSlots; ++k) {
        const float4 x = *reinterpret_cast<const float4*>(pp + (uint64_t)k * K);
        acc.x = acc.x + x.x;
        acc.y = acc.y + x.y;
        acc.z = acc.z + x.z;
        acc.w = acc.w + x.w;
        sum = sum + ps[k];
    }
    const uint64_t row = b * M + sp.dest;
    const bool dead = m[row] == -INFINITY;
    const float4 o = make_float4(attnDiv(acc.x, sum, dead), attnDiv(acc.y, sum, dead), attnDiv(acc.z, sum, dead),
                                 attnDiv(acc.w, sum, dead));
    if constexpr (MODE < 0) {
        *reinterpret_cast<float4*>(static_cast<float*>(Oout) + row * K + c) = o;
    } else {
        u32x2 o16;
        o16[0] = bwNarrow<MODE>(o.x, o.y);
        o16[1] = bwNarrow<MODE>(o.z, o.w);
        *reinterpret_cast<u32x2*>(static_cast<uint16_t*>(Oout) + row * K + c) = o16;
    }
    if (c == 0) sOut[row] = sum;
}

// D[b][r] = dO_r . O_r: 32 lanes per row (2 rows per wave, 8 per block).  MODE < 0: fp32 rows; 0 / 1: fp16 / bf16 rows
// widened exactly.  rows = b * M: the batch is folded into the row index.
template <int MODE>
__global__ void __launch_bounds__(256)
attnRowDot(const void* __restrict__ Oin, const void* __restrict__ dOin, float* __restrict__ D, uint64_t rows, uint32_t K) {
#pragma clang fp contract(off)
    const uint32_t l = threadIdx.x & 31u;
    const uint64_t r = (uint64_t)blockIdx.x * 8u + (threadIdx.x >> 5);
    float acc = 0.0f;
    if (r < rows) {
        if constexpr (MODE < 0) {
            const float* o = static_cast<const float*>(Oin) + r * K;
            const float* d = static_cast<const float*>(dOin) + r * K;
            for (uint32_t k = l; k < K; k += 32u) acc = fmaf(d[k], o[k], acc);
        } else {
            const uint16_t* o = static_cast<const uint16_t*>(Oin) + r * K;
            const uint16_t* d = static_cast<const uint16_t*>(dOin) + r * K;
            for (uint32_t k = l; k < K; k += 32u) {
                float ov, dv, unused;
                bwWiden<MODE>(o[k], ov, unused);
                bwWiden<MODE>(d[k], dv, unused);
                acc = fmaf(dv, ov, acc);
            }
        }
    }
    for (int off = 16; off; off >>= 1) acc = acc + __shfl_xor(acc, off, 64);   // (stays inside each half of the wave)
    if (r < rows && l == 0) D[r] = acc;
}

// one entry of the backward
__device__ __forceinline__ void attnEntryBackward(float scale, float p, float mr, float sr, float d, const float* dW,
                                                  float* dP, float* Wout, uint64_t t) {
#pragma clang fp contract(off)
    const float e = smExp(scale * p, mr);
    const float w = mr == -INFINITY ? 0.0f : e / sr;
    dP[t] = (w * (dW[t] - d)) * scale;
    Wout[t] = w;
}

// w, dP and W of every entry; the blocks as in attnRowMax (short rows by waves, then the chunk table's rows by blocks).
__global__ void __launch_bounds__(256)
attnValuesBackward(const uint32_t* __restrict__ ro, const BwSplit* __restrict__ splits, uint32_t M, uint32_t shortBlocks,
                   float scale, const float* __restrict__ P, const float* __restrict__ m, const float* __restrict__ s,
                   const float* __restrict__ D, const float* dW, float* dP, float* __restrict__ Wout, uint64_t nnz) {
    const uint64_t bM = (uint64_t)blockIdx.y * M;
    if (blockIdx.x >= shortBlocks) {
        const uint32_t row = splits[blockIdx.x - shortBlocks].dest;
        const uint32_t b = ro[row], n = ro[row + 1] - b;
        const uint64_t base = (uint64_t)blockIdx.y * nnz + b;
        const float mr = m[bM + row], sr = s[bM + row], d = D[bM + row];
        for (uint32_t i = threadIdx.x; i < n; i += 256u) attnEntryBackward(scale, P[base + i], mr, sr, d, dW, dP, Wout, base + i);
        return;
    }
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t r = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (r >= M) return;
    const uint32_t b = ro[r], n = ro[r + 1] - b;
    if (n == 0 || n > kSmChunk) return;
    const uint64_t base = (uint64_t)blockIdx.y * nnz + b;
    const float mr = m[bM + r], sr = s[bM + r], d = D[bM + r];
    for (uint32_t i = lane; i < n; i += 64u) attnEntryBackward(scale, P[base + i], mr, sr, d, dW, dP, Wout, base + i);
}

}  // namespace bsmr
