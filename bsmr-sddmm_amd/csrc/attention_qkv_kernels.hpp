// One-pass sparse attention (csrc/attention_qkv_capi.hpp, bsmr_sparse_attention_qkv_16; include/bsmr_hip.h "One-pass sparse
// attention"): O = softmax_rows(scale Q Kt^T over S's pattern) V without the scores ever reaching memory.
//
// attnQkv runs one wave per BwItem (a row of S, or one chunk of a row longer than BSMR_BACKWARD_CHUNK), 4 waves per
// block, batches in grid y.  The item's entries are taken in tiles of kQkvTile = 16 consecutive entries, and a tile is
// served by the 64 lanes in two layouts:
//   score layout  lane l serves entry l >> 2 of the tile, quarter l & 3.  Load i reads the 16 bytes at byte
//                 64 i + 16 (l & 3) of row Kt[c]: the four lanes of an entry read 64 contiguous bytes, K / 32 loads cover
//                 the row.  The lane's partial dot is ONE fp32 accumulator from +0 over its loads in ascending i, four
//                 dot2<MODE> per load in ascending k (16-bit products exact, fp32 accumulation); the four partials of an
//                 entry are added by two quad steps, x + lane^1 then x + lane^2 (fp32 addition commutes: the four lanes
//                 end with the same bits).  z = fl(scale p); a lane past the item's end holds -inf.
//   value layout  lane l owns the 16-bit pairs l + 64 i of the row of V (features 2 (l + 64 i) and the next), i < VC =
//                 ceil(Kv / 128): an entry's row is read as coalesced 256-byte pieces, lanes past Kv / 2 load nothing.
//                 e_j and c_j are broadcast in entry order (v_readlane), 4 source rows in flight as in attnGather16.
// Online softmax, wave-uniform (m, s: the same bits on every lane, as attnGather keeps its sum).  Before a tile:
//   m' = max(m, tile max) (NaN once any z was NaN);  if m' != m:  alpha = expf(fl(m - m')) (1 while m = -inf),
//   s = fl(s alpha), acc = fl(acc alpha);  then, in entry order, e_t = expf(fl(z_t - m')) (0 while m' = -inf),
//   s = s + e_t, acc_k = fmaf(e_t, V[c_t, k], acc_k).
// The column ids of 64 entries come from one coalesced load (the group after it is already in flight); the Kt loads of
// tile t + 1 are issued before the softmax and value phase of tile t and dotted behind it, so one tile of Kt is in
// registers at a time.  The Q row is loaded once per item: each lane keeps its K / 32 pieces in registers up to K = 128;
// wider rows are staged in the wave's own 1 KiB of LDS (the Kt tile alone takes 64 VGPRs at K = 512).
// Templates: MODE 0 / 1 = fp16 / bf16; NL = loads per Kt row the dot loop is unrolled for (1, 2, 4, 8, 16; K / 32 <= NL,
// a load past K / 32 repeats the row's last piece and its dot step is dropped by a select); VC as above (1, 2, 4).
//
// A direct item divides (IEEE), rounds once (bwNarrow) and stores O, m, s.  A chunk item stores (m_c, s_c, acc_c) to the
// workspace; attnQkvMerge merges them in chunk order: m = max_c m_c (NaN if any is), beta_c = expf(fl(m_c - m)) (0 when
// m_c = -inf: such a chunk is skipped), s = sum_c fl(s_c beta_c), acc = sum_c fl(acc_c beta_c) from +0; then the division and
// rounding.  A tile met while m is still -inf is skipped in the same way.
// No atomics, one writer per element, every address formed in 64 bits.  fp contraction is off and expf is the accurate one.
// The kernels live in a translation unit of their own (csrc/attention_qkv.hip), built without packed fp32 operations
// (v_pk_mul_f32 / v_pk_fma_f32); DESIGN.md 18 says what that buys in registers.
#pragma once

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "backward_lists.hpp"   // BwItem, BwSplit, kBwDirect
#include "lowp_device.hpp"      // u32x2, u32x4, dot2, ResidueLowp, bwWiden, bwNarrow
#include "softmax_device.hpp"   // attnDiv, smExp, smRowMax, smWaveSync

namespace bsmr {

constexpr uint32_t kQkvTile = 16;   // entries per tile: 64 lanes = 16 entries x 4 quarters of a Kt row

template <int MODE, int NL, int VC>
__global__ void __launch_bounds__(256)
attnQkv(const BwItem* __restrict__ items, uint32_t numItems, const uint32_t* __restrict__ src, float scale,
        const uint16_t* __restrict__ Q, const uint16_t* __restrict__ Kt, const uint16_t* __restrict__ V,
        uint16_t* __restrict__ O, float* __restrict__ mOut, float* __restrict__ sOut, float* __restrict__ partial,
        float* __restrict__ sPart, float* __restrict__ mPart, uint32_t K, uint32_t Kv, uint32_t M, uint32_t N,
        uint32_t numSlots) {
#pragma clang fp contract(off)
    constexpr bool QLDS = NL > 4;
    __shared__ u32x4 qLds[QLDS ? 4 * 64 : 1];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t it = (uint64_t)blockIdx.x * 4u + wave;
    if (it >= numItems) return;   // (whole waves leave: nothing below synchronises across waves)
    const BwItem item = items[it];
    const uint64_t b = blockIdx.y;
    const uint32_t quarter = lane & 3u, ent = lane >> 2, kc = K / 32u, pairs = Kv / 2u;
    const uint32_t len = item.end - item.begin, nt = (len + kQkvTile - 1u) / kQkvTile;
    const uint16_t* kb = Kt + b * N * K + quarter * 8u;
    const uint16_t* vb = V + b * N * Kv + 2u * lane;

    u32x4 q[QLDS ? 1 : NL] = {};
    if (nt) {   // (an empty row reads nothing: with nnz = 0 the operands may be NULL)
        const uint16_t* qr = Q + (b * M + item.dest) * K;
        if constexpr (QLDS) {
            if (lane < K / 8u) qLds[wave * 64u + lane] = *reinterpret_cast<const u32x4*>(qr + 8u * lane);
            smWaveSync();
        } else {
#pragma unroll
            for (int i = 0; i < NL; ++i)   // (a piece past K / 32 repeats the last one and is never dotted: no branch)
                q[i] = *reinterpret_cast<const u32x4*>(qr + 32u * min((uint32_t)i, kc - 1u) + 8u * quarter);
        }
    }
    // column ids of the item's entries [64 g, 64 g + 64), one per lane
    auto groupCols = [&](uint32_t g) -> uint32_t {
        const uint32_t e = g * 64u + lane;
        return e < len ? src[item.begin + e] : 0u;
    };
    // this lane's pieces of its entry's row of Kt in tile t; cols: the ids of the group tile t lies in
    auto loadKt = [&](uint32_t cols, uint32_t t, u32x4 (&kt)[NL]) {
        // Branch-free, so that the NL loads are in flight together: a lane past the item's end holds column 0 (groupCols)
        // and reads that row, a piece past K / 32 repeats the last one; neither is used.
        const uint32_t c = (uint32_t)__shfl((int)cols, (int)((t & 3u) * kQkvTile + ent), 64);
        const uint16_t* row = kb + (uint64_t)c * K;
#pragma unroll
        for (int i = 0; i < NL; ++i) kt[i] = *reinterpret_cast<const u32x4*>(row + 32u * min((uint32_t)i, kc - 1u));
    };
    // z of this lane's entry in tile t, the same bits on the entry's four lanes
    auto score = [&](const u32x4 (&kt)[NL], uint32_t t) -> float {
        float p = 0.0f;
#pragma unroll
        for (int i = 0; i < NL; ++i) {
            u32x4 qi;
            if constexpr (QLDS) qi = qLds[wave * 64u + 4u * min((uint32_t)i, kc - 1u) + quarter];
            else qi = q[i];
            const float next = ResidueLowp<MODE>::dot(qi, kt[i], p);
            p = (uint32_t)i < kc ? next : p;   // (wave-uniform select: the chain has exactly K / 32 steps)
        }
        p = p + __shfl_xor(p, 1, 64);
        p = p + __shfl_xor(p, 2, 64);
        return t * kQkvTile + ent < len ? scale * p : -INFINITY;
    };
    auto loadV = [&](uint32_t c, uint32_t (&x)[VC]) {
        const uint16_t* row = vb + (uint64_t)c * Kv;
#pragma unroll
        for (int i = 0; i < VC; ++i) x[i] = lane + 64u * i < pairs ? *reinterpret_cast<const uint32_t*>(row + 128u * i) : 0u;
    };
    float acc[2 * VC];
#pragma unroll
    for (int i = 0; i < 2 * VC; ++i) acc[i] = 0.0f;
    auto fmaV = [&](float w, const uint32_t (&x)[VC]) {
#pragma unroll
        for (int i = 0; i < VC; ++i) {
            float lo, hi;
            bwWiden<MODE>(x[i], lo, hi);
            acc[2 * i] = fmaf(w, lo, acc[2 * i]);
            acc[2 * i + 1] = fmaf(w, hi, acc[2 * i + 1]);
        }
    };

    float m = -INFINITY, s = 0.0f;
    bool nan = false;
    if (nt) {
        uint32_t cV = groupCols(0), cK = cV, cNext = groupCols(1);
        u32x4 kt[NL] = {};
        loadKt(cK, 0, kt);
        float z = score(kt, 0);
        for (uint32_t t = 0; t < nt; ++t) {
            const bool more = t + 1u < nt;
            if (more) {   // tile t + 1's rows of Kt fly during tile t's softmax and value phase
                if (((t + 1u) & 3u) == 0) {
                    cK = cNext;
                    cNext = groupCols((t + 1u) / 4u + 1u);
                }
                loadKt(cK, t + 1u, kt);
            }
            float tm = z;
            for (int o = 32; o >= 4; o >>= 1) tm = fmaxf(tm, __shfl_xor(tm, o, 64));   // (the 4 lanes of a quad agree)
            nan |= __any(z != z) != 0;
            const float mNew = smRowMax(fmaxf(m, tm), nan);
            if (mNew != m) {   // wave-uniform (a NaN keeps rescaling: the row stays NaN)
                if (m != -INFINITY) {
                    const float alpha = expf(m - mNew);
                    s = s * alpha;
#pragma unroll
                    for (int i = 0; i < 2 * VC; ++i) acc[i] = acc[i] * alpha;
                }
                m = mNew;
            }
            const uint32_t e = __float_as_uint(smExp(z, m));
            // While m = -inf every e so far is 0: the tile's value phase is skipped, so that a non-finite row of V behind a
            // -inf score cannot reach acc as 0 * inf (finite rows of V: the same bits, acc stays +0 and s stays 0).
            const uint32_t n = m == -INFINITY ? 0u : min(kQkvTile, len - t * kQkvTile), base = (t & 3u) * kQkvTile;
            uint32_t j = 0;
            for (; j + 4u <= n; j += 4u) {
                const uint32_t c0 = __builtin_amdgcn_readlane(cV, base + j), c1 = __builtin_amdgcn_readlane(cV, base + j + 1u);
                const uint32_t c2 = __builtin_amdgcn_readlane(cV, base + j + 2u), c3 = __builtin_amdgcn_readlane(cV, base + j + 3u);
                const float w0 = __uint_as_float(__builtin_amdgcn_readlane(e, 4u * j));
                const float w1 = __uint_as_float(__builtin_amdgcn_readlane(e, 4u * j + 4u));
                const float w2 = __uint_as_float(__builtin_amdgcn_readlane(e, 4u * j + 8u));
                const float w3 = __uint_as_float(__builtin_amdgcn_readlane(e, 4u * j + 12u));
                uint32_t x0[VC], x1[VC], x2[VC], x3[VC];
                loadV(c0, x0);
                loadV(c1, x1);
                loadV(c2, x2);
                loadV(c3, x3);
                s = s + w0;
                s = s + w1;
                s = s + w2;
                s = s + w3;
                fmaV(w0, x0);
                fmaV(w1, x1);
                fmaV(w2, x2);
                fmaV(w3, x3);
            }
            for (; j < n; ++j) {
                const uint32_t cj = __builtin_amdgcn_readlane(cV, base + j);
                const float wj = __uint_as_float(__builtin_amdgcn_readlane(e, 4u * j));
                uint32_t xj[VC];
                loadV(cj, xj);
                s = s + wj;
                fmaV(wj, xj);
            }
            if (more) z = score(kt, t + 1u);
            if (((t + 1u) & 3u) == 0) cV = cK;
        }
    }
    if (item.slot == kBwDirect) {   // the one store of a finished row
        const bool dead = m == -INFINITY;   // an empty row, or every score -inf: s = 0
        const uint64_t row = b * M + item.dest;
        uint16_t* o = O + row * Kv + 2u * lane;
#pragma unroll
        for (int i = 0; i < VC; ++i)
            if (lane + 64u * i < pairs)
                *reinterpret_cast<uint32_t*>(o + 128u * i) =
                    bwNarrow<MODE>(attnDiv(acc[2 * i], s, dead), attnDiv(acc[2 * i + 1], s, dead));
        if (lane == 0) {
            mOut[row] = m;
            sOut[row] = s;
        }
    } else {
        const uint64_t slot = b * numSlots + item.slot;
        float* p = partial + slot * Kv + 2u * lane;
#pragma unroll
        for (int i = 0; i < VC; ++i)
            if (lane + 64u * i < pairs) *reinterpret_cast<float2*>(p + 128u * i) = make_float2(acc[2 * i], acc[2 * i + 1]);
        if (lane == 0) {
            mPart[slot] = m;
            sPart[slot] = s;
        }
    }
}

// A split row: the max-aware merge of its chunks' (m_c, s_c, acc_c) in chunk order, then the division and the one
// rounding; one thread per 4 features of the row (every thread of a row repeats the row's scalar chain: same bits).
template <int MODE>
__global__ void __launch_bounds__(256)
attnQkvMerge(const BwSplit* __restrict__ splits, uint32_t numSplits, const float* __restrict__ partial,
             const float* __restrict__ sPart, const float* __restrict__ mPart, uint16_t* __restrict__ O,
             float* __restrict__ mOut, float* __restrict__ sOut, uint32_t Kv, uint32_t M, uint32_t numSlots) {
#pragma clang fp contract(off)
    const uint32_t q = Kv / 4u;
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= (uint64_t)numSplits * q) return;
    const BwSplit sp = splits[i / q];
    const uint64_t c = (i % q) * 4u;
    const uint64_t b = blockIdx.y, first = b * numSlots + sp.firstSlot;
    const float* pp = partial + first * Kv + c;
    const float* ps = sPart + first;
    const float* pm = mPart + first;
    float m = -INFINITY;
    bool nan = false;
    for (uint32_t k = 0; k < sp.numSlots; ++k) {
        const float mk = pm[k];
        m = fmaxf(m, mk);
        nan |= mk != mk;
    }
    m = smRowMax(m, nan);
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    float s = 0.0f;
    for (uint32_t k = 0; k < sp.numSlots; ++k) {
        const float mk = pm[k];
        if (mk == -INFINITY) continue;   // beta = 0: the chunk is skipped, not multiplied (its acc_c is +0 or never used)
        const float beta = expf(mk - m);
        const float4 x = *reinterpret_cast<const float4*>(pp + (uint64_t)k * Kv);
        s = s + ps[k] * beta;
        acc.x = acc.x + x.x * beta;
        acc.y = acc.y + x.y * beta;
        acc.z = acc.z + x.z * beta;
        acc.w = acc.w + x.w * beta;
    }
    const uint64_t row = b * M + sp.dest;
    const bool dead = m == -INFINITY;
    u32x2 o16;
    o16[0] = bwNarrow<MODE>(attnDiv(acc.x, s, dead), attnDiv(acc.y, s, dead));
    o16[1] = bwNarrow<MODE>(attnDiv(acc.z, s, dead), attnDiv(acc.w, s, dead));
    *reinterpret_cast<u32x2*>(O + row * Kv + c) = o16;
    if (c == 0) {
        mOut[row] = m;
        sOut[row] = s;
    }
}

}  // namespace bsmr
