// Row softmax over S's pattern and its backward (csrc/softmax_capi.hpp, bsmr_sparse_softmax / _backward).
//
// Values are in S's CSR order; row r owns positions [ro[r], ro[r+1]).  Per row, in this op order (no contraction: the
// kernels turn fp contraction off with a pragma, so every step below is one IEEE-rounded fp32 operation):
//   forward   z_t = fl32(scale * x_t);  m = max_t z_t;  e_t = expf(z_t - m);  s = sum_t e_t;  y_t = e_t / s
//   backward  g = sum_t y_t * dY_t (fma chain);  dX_t = fl32(fl32(y_t * fl32(dY_t - g)) * scale)
// Summation order of s and g (a function of the pattern alone): a sequential fp32 chain in CSR order starting from +0
// (s: acc = acc + e_t; g: acc = fmaf(y_t, dY_t, acc)); a row longer than BSMR_BACKWARD_CHUNK is summed chunk by chunk
// and the partials are added in chunk order (p0 + p1 + ...): the order of bsmr_spmm, i.e. oracle_gather_twin at K = 1.
// Special values: a NaN z makes m NaN (fmaxf alone would drop it), so the whole row is NaN; +inf gives m = +inf and
// inf - inf = NaN, so the row is NaN too; m = -inf (every entry -inf) gives exact zeros; other -inf entries give exp = 0.
//
// Length classes: a row of at most BSMR_BACKWARD_CHUNK entries is one wave's (softmaxShort / softmaxShortBackward):
// the row is read once into registers (8 entries per lane), staged in LDS for the chain, which lane 0 runs while the
// other waves of the SIMD proceed, and written once.  A longer row is one workgroup's (softmaxLong / _Backward, one
// block per entry of the handle's row chunk table): the forward writes e into Y and rescales it in place, the chains
// (one thread per chunk) re-read e or (y, dY) from the block's own writes, which the CU's L1 keeps coherent within a
// workgroup.  Nothing needs workspace; the chunk partials stay in LDS.
// Y may alias X and dX may alias dY: every position is read before it is written, by the thread that writes it or
// behind a barrier, so no pointer is __restrict__.  All addresses are formed in 64 bits (the batch multiplies nnz).
#pragma once

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "spmm_kernels.hpp"

namespace bsmr {

constexpr uint32_t kSmChunk = BSMR_BACKWARD_CHUNK;
constexpr uint32_t kSmPerLane = kSmChunk / 64u;   // entries of a short row held by one lane

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

// ---- rows of 1 .. kSmChunk entries: one wave per row, 4 rows per block ----
__global__ void __launch_bounds__(256)
softmaxShort(const uint32_t* __restrict__ ro, uint32_t M, float scale, const float* X, float* Y, uint64_t nnz) {
#pragma clang fp contract(off)
    __shared__ float lds[4][kSmChunk];
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    const uint32_t r = blockIdx.x * 4u + w;
    if (r >= M) return;
    const uint32_t b = ro[r], n = ro[r + 1] - b;
    if (n == 0 || n > kSmChunk) return;   // (long rows: softmaxLong)
    const uint64_t base = (uint64_t)blockIdx.y * nnz + b;
    float z[kSmPerLane];
    float m = -INFINITY;
    bool nan = false;
#pragma unroll
    for (uint32_t k = 0; k < kSmPerLane; ++k) {
        const uint32_t i = lane + 64u * k;
        z[k] = i < n ? scale * X[base + i] : -INFINITY;
        m = fmaxf(m, z[k]);
        nan |= z[k] != z[k];
    }
    m = smRowMax(smWaveMax(m), __any(nan));
    float* e = lds[w];
#pragma unroll
    for (uint32_t k = 0; k < kSmPerLane; ++k) {
        const uint32_t i = lane + 64u * k;
        z[k] = smExp(z[k], m);
        if (i < n) e[i] = z[k];
    }
    smWaveSync();
    float s = 0.0f;
    if (lane == 0) {
        float acc = 0.0f;
#pragma unroll 8
        for (uint32_t t = 0; t < n; ++t) acc = acc + e[t];
        s = acc;
    }
    s = __shfl(s, 0, 64);
#pragma unroll
    for (uint32_t k = 0; k < kSmPerLane; ++k) {
        const uint32_t i = lane + 64u * k;
        if (i < n) Y[base + i] = m == -INFINITY ? 0.0f : z[k] / s;   // (s = 0 there)
    }
}

__global__ void __launch_bounds__(256)
softmaxShortBackward(const uint32_t* __restrict__ ro, uint32_t M, float scale, const float* Yv, const float* dY,
                     float* dX, uint64_t nnz) {
#pragma clang fp contract(off)
    __shared__ float lds[4][2][kSmChunk];
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    const uint32_t r = blockIdx.x * 4u + w;
    if (r >= M) return;
    const uint32_t b = ro[r], n = ro[r + 1] - b;
    if (n == 0 || n > kSmChunk) return;
    const uint64_t base = (uint64_t)blockIdx.y * nnz + b;
    float y[kSmPerLane], d[kSmPerLane];
    float* ly = lds[w][0];
    float* ld = lds[w][1];
#pragma unroll
    for (uint32_t k = 0; k < kSmPerLane; ++k) {
        const uint32_t i = lane + 64u * k;
        y[k] = i < n ? Yv[base + i] : 0.0f;
        d[k] = i < n ? dY[base + i] : 0.0f;
        if (i < n) {
            ly[i] = y[k];
            ld[i] = d[k];
        }
    }
    smWaveSync();
    float g = 0.0f;
    if (lane == 0) {
        float acc = 0.0f;
#pragma unroll 8
        for (uint32_t t = 0; t < n; ++t) acc = fmaf(ly[t], ld[t], acc);
        g = acc;
    }
    g = __shfl(g, 0, 64);
#pragma unroll
    for (uint32_t k = 0; k < kSmPerLane; ++k) {
        const uint32_t i = lane + 64u * k;
        if (i < n) dX[base + i] = (y[k] * (d[k] - g)) * scale;
    }
}

// ---- rows of more than kSmChunk entries: one block of 256 per row (the handle's row chunk table) ----
__device__ __forceinline__ float smBlockMax(float m, bool nan, float* red) {
    m = smRowMax(smWaveMax(m), __any(nan));   // NaN survives fmaxf only through the flag, so fold it in per wave ...
    if ((threadIdx.x & 63u) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    float r = red[0];
    bool n = r != r;
    for (int i = 1; i < 4; ++i) {              // ... and again across the waves
        r = fmaxf(r, red[i]);
        n |= red[i] != red[i];
    }
    __syncthreads();
    return smRowMax(r, n);
}

// The chunk partials of one row in chunk order: thread k of a round chains chunk (round * 256 + k) with chain(t0, t1);
// thread 0 adds the round's partials to the running sum.  Returns the sum on every thread.
template <typename Chain>
__device__ __forceinline__ float smChunkSum(uint32_t n, float* part, Chain chain) {
#pragma clang fp contract(off)
    const uint32_t chunks = (n + kSmChunk - 1u) / kSmChunk;
    float total = 0.0f;
    for (uint32_t c0 = 0; c0 < chunks; c0 += 256u) {
        const uint32_t c = c0 + threadIdx.x;
        if (c < chunks) part[threadIdx.x] = chain(c * kSmChunk, (uint32_t)min((uint64_t)n, (c + 1ull) * kSmChunk));
        __syncthreads();
        if (threadIdx.x == 0) {
            float acc = c0 == 0 ? part[0] : total + part[0];
            for (uint32_t k = 1; k < min(256u, chunks - c0); ++k) acc = acc + part[k];
            part[256] = acc;
        }
        __syncthreads();
        total = part[256];
        __syncthreads();
    }
    return total;
}

__global__ void __launch_bounds__(256)
softmaxLong(const uint32_t* __restrict__ ro, const BwSplit* __restrict__ splits, float scale, const float* X, float* Y,
            uint64_t nnz) {
#pragma clang fp contract(off)
    __shared__ float part[257];
    __shared__ float red[4];
    const uint32_t row = splits[blockIdx.x].dest;
    const uint32_t b = ro[row], n = ro[row + 1] - b;
    const uint64_t base = (uint64_t)blockIdx.y * nnz + b;
    float m = -INFINITY;
    bool nan = false;
    for (uint32_t i = threadIdx.x; i < n; i += 256u) {
        const float z = scale * X[base + i];
        m = fmaxf(m, z);
        nan |= z != z;
    }
    m = smBlockMax(m, nan, red);
    for (uint32_t i = threadIdx.x; i < n; i += 256u) Y[base + i] = smExp(scale * X[base + i], m);
    __syncthreads();   // e is read back by other threads of this block: coherent through the CU's L1
    const float* e = Y + base;
    const float s = smChunkSum(n, part, [&](uint32_t t0, uint32_t t1) {
        float acc = 0.0f;
        for (uint32_t t = t0; t < t1; ++t) acc = acc + e[t];
        return acc;
    });
    if (m == -INFINITY) return;   // e = 0 is the result (s = 0)
    for (uint32_t i = threadIdx.x; i < n; i += 256u) Y[base + i] = Y[base + i] / s;
}

__global__ void __launch_bounds__(256)
softmaxLongBackward(const uint32_t* __restrict__ ro, const BwSplit* __restrict__ splits, float scale, const float* Yv,
                    const float* dY, float* dX, uint64_t nnz) {
#pragma clang fp contract(off)
    __shared__ float part[257];
    const uint32_t row = splits[blockIdx.x].dest;
    const uint32_t b = ro[row], n = ro[row + 1] - b;
    const uint64_t base = (uint64_t)blockIdx.y * nnz + b;
    const float* y = Yv + base;
    const float* d = dY + base;
    const float g = smChunkSum(n, part, [&](uint32_t t0, uint32_t t1) {
        float acc = 0.0f;
        for (uint32_t t = t0; t < t1; ++t) acc = fmaf(y[t], d[t], acc);
        return acc;
    });   // (its last barrier orders every read of dY before the first write of dX)
    for (uint32_t i = threadIdx.x; i < n; i += 256u) dX[base + i] = (y[i] * (d[i] - g)) * scale;
}

}  // namespace bsmr
