// One-pass sparse attention on a quantised KV cache (csrc/attention_qkv_kv_capi.hpp, bsmr_sparse_attention_qkv_kv8 / _kv8_mx
// / _kv4_mx; include/bsmr_hip.h "One-pass sparse attention on fp8, MXFP8 and MXFP4 keys and values"):
// attnQkv (csrc/attention_qkv_kernels.hpp) with Kt and V read as the cache holds them - OCP fp8 bytes or e2m1 nibbles,
// with or without E8M0 block scales - and widened in registers.  No 16-bit copy of Kt, no score array.
//
// The work split is attnQkv's: one wave per BwItem, 4 waves per block, batches in grid y; tiles of kQkvTile = 16 entries;
// the Kt loads of tile t + 1 in flight behind tile t's softmax and value phase; column ids by one coalesced load,
// ds_bpermute into the score layout and v_readlane into the value layout; the same online-softmax statements, -inf / NaN
// guards, direct store and chunk partials in the same workspace layout (attnQkvMerge merges them, unchanged).
// What differs is how Kt and V reach the arithmetic.  FMT 0 / 1 / 2 = e4m3fn / e5m2 / e2m1, MX = block scales (always
// with e2m1); CB = code bytes per 8 elements: 8 (fp8) or 4 (fp4).
//   score layout  lane l serves entry l >> 2, quarter j = l & 3, and owns the elements 32 i + 8 j ... 32 i + 8 j + 7 of
//                 Kt[c], as in attnQkv: piece i is ONE load of CB bytes at byte (32 i + 8 j) CB / 8 of the row, so the four
//                 lanes of an entry read one contiguous block of 32 elements.  The codes are widened two at a time to a
//                 packed 16-bit pair of MODE's format (v_cvt_scalef32_pk_{f16,bf16}_{fp8,bf8,fp4}, the instruction's
//                 scale operand fixed at 1.0: every code is a value of both 16-bit formats, the widening is exact) and
//                 fed to dot2<MODE> against the lane's piece of Q.
//                 Without scales the lane runs ONE fp32 accumulator from +0 over its pieces, four dot2 per piece in
//                 ascending k: attnQkv's chain on the widened operand, bit for bit.
//                 With scales block i has a fresh accumulator d_i from +0 (four dot2), then p = fmaf(d_i, sc_i, p) with
//                 sc_i = bwScaleMx(Es[c][i]); the scale never enters a 16-bit value.  One scale byte load per piece and
//                 lane (the four lanes of an entry load the same byte), in flight with the piece.
//                 Then the two quad steps and z = fl(scale p) as in attnQkv.
//   value layout  lane l owns the VE consecutive features VE l + 64 VE i, i < VC: VE = 4 (fp8), VC = ceil(Kv / 256) in
//                 {1, 2}; VE = 8 (fp4), VC = 1.  Either way that is one 32-bit load at byte 4 l + 256 i of the row and one
//                 scale byte (the VE features lie in one block of 32); a lane whose bytes lie past the row loads nothing.
//                 x = widen(code) (bwWiden8 / bwWiden4, exact fp32), with scales x = fl(widen(code) sc): attnGather8 /
//                 attnGather4's element.  acc_k = fmaf(e_t, x, acc_k) in entry order on one lane from +0, 4 source rows
//                 in flight; s never sees the scales.  A finished row stores VE 16-bit elements per lane and chunk (8 or
//                 16 bytes), a chunk item VE floats.
// Q is loaded as in attnQkv: K / 32 pieces of 16 bytes per lane in registers up to K = 128, the wave's own 1 KiB of LDS
// above (it is the same 16-bit row; only the Kt tile shrank).
// Every byte address is formed in 64 bits: rows of K CB / 8 bytes and K / 32 scale bytes, batches of N rows.
// Built like attnQkv, in a translation unit without packed fp32 operations (csrc/attention_qkv_kv.hip, QKV_FLAGS).
#pragma once

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "attention_qkv_kernels.hpp"   // kQkvTile; attnDiv, smExp, smRowMax, smWaveSync, BwItem, bwNarrow, dot2
#include "quant_device.hpp"            // bwWiden8, bwWiden4, bwScaleMx

namespace bsmr {

// Two codes of `word` as a packed pair of MODE's 16-bit format, the first code in the low half.  SEL: the 16-bit half of
// the word (fp8: 0, 1) or its byte (fp4: 0 .. 3) the two codes lie in.  Exact: the scale operand is 1.0.
template <int MODE, int FMT, int SEL>
__device__ __forceinline__ uint32_t qkvPair(uint32_t word) {
    if constexpr (MODE == 0) {
        typedef _Float16 h2 __attribute__((ext_vector_type(2)));
        h2 r;
        if constexpr (FMT == 0) r = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(word, 1.0f, SEL != 0);
        else if constexpr (FMT == 1) r = __builtin_amdgcn_cvt_scalef32_pk_f16_bf8(word, 1.0f, SEL != 0);
        else r = __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(word, 1.0f, SEL);
        return __builtin_bit_cast(uint32_t, r);
    } else {
        typedef __bf16 b2 __attribute__((ext_vector_type(2)));
        b2 r;
        if constexpr (FMT == 0) r = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(word, 1.0f, SEL != 0);
        else if constexpr (FMT == 1) r = __builtin_amdgcn_cvt_scalef32_pk_bf16_bf8(word, 1.0f, SEL != 0);
        else r = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(word, 1.0f, SEL);
        return __builtin_bit_cast(uint32_t, r);
    }
}

// A lane's piece of a row of Kt: 8 codes - two words of fp8 bytes, one word of e2m1 nibbles
template <int FMT> struct QkvPiece { using T = u32x2; };
template <> struct QkvPiece<2> { using T = uint32_t; };

// the 8 codes of a piece as the four 16-bit pairs dot2<MODE> takes, in element order
template <int MODE, int FMT>
__device__ __forceinline__ u32x4 qkvWiden(const typename QkvPiece<FMT>::T& x) {
    u32x4 r;
    if constexpr (FMT == 2) {
        r[0] = qkvPair<MODE, 2, 0>(x);
        r[1] = qkvPair<MODE, 2, 1>(x);
        r[2] = qkvPair<MODE, 2, 2>(x);
        r[3] = qkvPair<MODE, 2, 3>(x);
    } else {
        r[0] = qkvPair<MODE, FMT, 0>(x[0]);
        r[1] = qkvPair<MODE, FMT, 1>(x[0]);
        r[2] = qkvPair<MODE, FMT, 0>(x[1]);
        r[3] = qkvPair<MODE, FMT, 1>(x[1]);
    }
    return r;
}

// NL: pieces per Kt row the dot loop is unrolled for, as in attnQkv (K / 32 <= NL; a piece past K / 32 repeats the row's
// last one and its step is dropped by a select).  Ks / Vs: the E8M0 scales [b][N][K / 32] and [b][N][Kv / 32], read only
// with MX.
template <int MODE, int FMT, bool MX, int NL, int VC>
__global__ void __launch_bounds__(256)
attnQkvKv(const BwItem* __restrict__ items, uint32_t numItems, const uint32_t* __restrict__ src, float scale,
          const uint16_t* __restrict__ Q, const uint8_t* __restrict__ Kt, const uint8_t* __restrict__ Ks,
          const uint8_t* __restrict__ V, const uint8_t* __restrict__ Vs, uint16_t* __restrict__ O, float* __restrict__ mOut,
          float* __restrict__ sOut, float* __restrict__ partial, float* __restrict__ sPart, float* __restrict__ mPart,
          uint32_t K, uint32_t Kv, uint32_t M, uint32_t N, uint32_t numSlots) {
#pragma clang fp contract(off)
    static_assert(FMT != 2 || (MX && VC == 1), "e2m1 always carries block scales; one value chunk covers Kv = 512");
    constexpr bool QLDS = NL > 4;
    constexpr uint32_t CB = FMT == 2 ? 4u : 8u;   // code bytes per 8 elements
    constexpr int VE = FMT == 2 ? 8 : 4;          // features per lane and value chunk: one 32-bit word of codes
    using Piece = typename QkvPiece<FMT>::T;
    __shared__ u32x4 qLds[QLDS ? 4 * 64 : 1];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t it = (uint64_t)blockIdx.x * 4u + wave;
    if (it >= numItems) return;   // (whole waves leave: nothing below synchronises across waves)
    const BwItem item = items[it];
    const uint64_t b = blockIdx.y;
    const uint32_t quarter = lane & 3u, ent = lane >> 2, kc = K / 32u, vc = Kv / 32u;
    const uint32_t kRow = K / 8u * CB, vRow = Kv / 8u * CB;   // bytes per row of Kt, of V
    const uint32_t len = item.end - item.begin, nt = (len + kQkvTile - 1u) / kQkvTile;
    const uint8_t* kb = Kt + b * N * kRow + quarter * CB;
    const uint8_t* ksb = MX ? Ks + b * N * kc : nullptr;
    const uint8_t* vb = V + b * N * vRow + 4u * lane;
    const uint8_t* vsb = MX ? Vs + b * N * vc + (uint32_t)VE * lane / 32u : nullptr;

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
    // this lane's pieces of its entry's row of Kt in tile t and their scale codes; cols: the ids of the group tile t lies in
    auto loadKt = [&](uint32_t cols, uint32_t t, Piece (&kt)[NL], uint32_t (&ks)[MX ? NL : 1]) {
        // Branch-free, so that the loads are in flight together: a lane past the item's end holds column 0 (groupCols)
        // and reads that row, a piece past K / 32 repeats the last one; neither is used.
        const uint32_t c = (uint32_t)__shfl((int)cols, (int)((t & 3u) * kQkvTile + ent), 64);
        const uint8_t* row = kb + (uint64_t)c * kRow;
#pragma unroll
        for (int i = 0; i < NL; ++i) kt[i] = *reinterpret_cast<const Piece*>(row + 4u * CB * min((uint32_t)i, kc - 1u));
        if constexpr (MX) {
            const uint8_t* es = ksb + (uint64_t)c * kc;
#pragma unroll
            for (int i = 0; i < NL; ++i) ks[i] = es[min((uint32_t)i, kc - 1u)];
        }
    };
    // z of this lane's entry in tile t, the same bits on the entry's four lanes
    auto score = [&](const Piece (&kt)[NL], const uint32_t (&ks)[MX ? NL : 1], uint32_t t) -> float {
        float p = 0.0f;
#pragma unroll
        for (int i = 0; i < NL; ++i) {
            u32x4 qi;
            if constexpr (QLDS) qi = qLds[wave * 64u + 4u * min((uint32_t)i, kc - 1u) + quarter];
            else qi = q[i];
            const u32x4 ki = qkvWiden<MODE, FMT>(kt[i]);
            float next;
            if constexpr (MX) next = fmaf(ResidueLowp<MODE>::dot(qi, ki, 0.0f), bwScaleMx(ks[i]), p);
            else next = ResidueLowp<MODE>::dot(qi, ki, p);
            p = (uint32_t)i < kc ? next : p;   // (wave-uniform select: the chain has exactly K / 32 steps)
        }
        p = p + __shfl_xor(p, 1, 64);
        p = p + __shfl_xor(p, 2, 64);
        return t * kQkvTile + ent < len ? scale * p : -INFINITY;
    };
    // a source row of V: this lane's word of codes per value chunk and, with MX, its scale code
    struct VRow {
        uint32_t x[VC], e[MX ? VC : 1];
    };
    auto loadV = [&](uint32_t c, VRow& r) {
        const uint8_t* row = vb + (uint64_t)c * vRow;
#pragma unroll
        for (int i = 0; i < VC; ++i) {
            const bool on = 4u * lane + 256u * i < vRow;
            r.x[i] = on ? *reinterpret_cast<const uint32_t*>(row + 256u * i) : 0u;
            if constexpr (MX) r.e[i] = on ? vsb[(uint64_t)c * vc + (64u * VE / 32u) * i] : 127u;
        }
    };
    float acc[VE * VC];
#pragma unroll
    for (int i = 0; i < VE * VC; ++i) acc[i] = 0.0f;
    auto fmaV = [&](float w, const VRow& r) {
#pragma unroll
        for (int i = 0; i < VC; ++i) {
            float x[VE];
            if constexpr (FMT == 2) bwWiden4(r.x[i], x);
            else bwWiden8<FMT>(r.x[i], x);
            if constexpr (MX) {
                const float sc = bwScaleMx(r.e[i]);
#pragma unroll
                for (int k = 0; k < VE; ++k) acc[VE * i + k] = fmaf(w, x[k] * sc, acc[VE * i + k]);
            } else {
#pragma unroll
                for (int k = 0; k < VE; ++k) acc[VE * i + k] = fmaf(w, x[k], acc[VE * i + k]);
            }
        }
    };

    float m = -INFINITY, s = 0.0f;
    bool nan = false;
    if (nt) {
        uint32_t cV = groupCols(0), cK = cV, cNext = groupCols(1);
        Piece kt[NL] = {};
        uint32_t ks[MX ? NL : 1] = {};
        loadKt(cK, 0, kt, ks);
        float z = score(kt, ks, 0);
        for (uint32_t t = 0; t < nt; ++t) {
            const bool more = t + 1u < nt;
            if (more) {   // tile t + 1's rows of Kt fly during tile t's softmax and value phase
                if (((t + 1u) & 3u) == 0) {
                    cK = cNext;
                    cNext = groupCols((t + 1u) / 4u + 1u);
                }
                loadKt(cK, t + 1u, kt, ks);
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
                    for (int i = 0; i < VE * VC; ++i) acc[i] = acc[i] * alpha;
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
                VRow x0, x1, x2, x3;
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
                VRow xj;
                loadV(cj, xj);
                s = s + wj;
                fmaV(wj, xj);
            }
            if (more) z = score(kt, ks, t + 1u);
            if (((t + 1u) & 3u) == 0) cV = cK;
        }
    }
    const uint32_t f0 = (uint32_t)VE * lane;   // this lane's first feature of value chunk 0; chunk i: + 64 VE i
    if (item.slot == kBwDirect) {   // the one store of a finished row
        const bool dead = m == -INFINITY;   // an empty row, or every score -inf: s = 0
        const uint64_t row = b * M + item.dest;
        uint16_t* o = O + row * Kv + f0;
#pragma unroll
        for (int i = 0; i < VC; ++i)
            if (f0 + 64u * VE * i < Kv) {
                uint32_t w[VE / 2];
#pragma unroll
                for (int k = 0; k < VE / 2; ++k)
                    w[k] = bwNarrow<MODE>(attnDiv(acc[VE * i + 2 * k], s, dead), attnDiv(acc[VE * i + 2 * k + 1], s, dead));
                if constexpr (VE == 8) {
                    u32x4 o16 = {w[0], w[1], w[2], w[3]};
                    *reinterpret_cast<u32x4*>(o + 64u * VE * i) = o16;
                } else {
                    u32x2 o16 = {w[0], w[1]};
                    *reinterpret_cast<u32x2*>(o + 64u * VE * i) = o16;
                }
            }
        if (lane == 0) {
            mOut[row] = m;
            sOut[row] = s;
        }
    } else {
        const uint64_t slot = b * numSlots + item.slot;
        float* p = partial + slot * Kv + f0;
#pragma unroll
        for (int i = 0; i < VC; ++i)
            if (f0 + 64u * VE * i < Kv) {
#pragma unroll
                for (int k = 0; k < VE; k += 4)
                    *reinterpret_cast<float4*>(p + 64u * VE * i + k) =
                        make_float4(acc[VE * i + k], acc[VE * i + k + 1], acc[VE * i + k + 2], acc[VE * i + k + 3]);
            }
        if (lane == 0) {
            mPart[slot] = m;
            sPart[slot] = s;
        }
    }
}

}  // namespace bsmr
