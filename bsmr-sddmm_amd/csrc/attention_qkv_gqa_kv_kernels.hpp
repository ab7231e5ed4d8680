// One-pass sparse attention with grouped key/value heads on a quantised KV cache (csrc/attention_qkv_gqa_kv_capi.hpp,
// bsmr_sparse_attention_qkv_gqa_kv8 / _kv8_mx / _kv4_mx; include/bsmr_hip.h "One-pass grouped-head sparse attention on fp8,
// MXFP8 and MXFP4 keys and values"): b query heads read b / g key/value heads whose Kt and V are OCP fp8 bytes
// or e2m1 nibbles, with or without E8M0 block scales, as the cache holds them.  Query head h reads KV head h / g.
//
// The work split is attnQkvGqa's (csrc/attention_qkv_gqa_kernels.hpp): one wave per BwItem and sub-group of G consecutive
// heads of a KV group, 4 waves per block, grid y = (b / g) * ceil(g / G); a sub-group that ends past the group clamps its
// surplus heads to the group's last head, and those store nothing.  The operand path is attnQkvKv's
// (csrc/attention_qkv_kv_kernels.hpp), paid once per wave instead of once per head:
//   score   per tile of kQkvTile = 16 entries the wave loads the column ids, the lane's code pieces of its entry's row of Kt
//           (u32x2 per piece for fp8, one word for e2m1) and, with MX, one scale byte per piece ONCE.  Piece i is widened
//           ONCE to the four 16-bit pairs of MODE's format (qkvWiden: four v_cvt_scalef32_pk_*, exact) and all G heads are
//           dotted against that register - piece outer, head inner, one widened piece live at a time.  Without scales head
//           h runs one accumulator chain p_h over its pieces; with scales block i gets a fresh d from +0 per head and
//           p_h = fmaf(d, bwScaleMx(ks_i), p_h): attnQkvKv's statements, per head.
//   value   per entry the lane's word of V codes (4 features of fp8 on 64 lanes, 8 of e2m1 on the lanes below Kv / 8: one
//           value chunk covers Kv <= 256 in every format) and its scale byte are loaded ONCE, 4 rows in flight, widened ONCE
//           (bwWiden8 / bwWiden4) and with MX multiplied ONCE, x = fl(widen sc).  The fp32 x[VE] then feeds G groups of
//           fmaf(w_h, x, acc_h), w_h read from e_h by v_readlane.  The "skip while m_h = -inf" rule is per head, behind
//           the wave-uniform `live` mask, as in attnQkvGqa.
// Contract: every head runs attnQkvKv's statement sequence on the same values (x = fl(widen sc) is the same IEEE product
// whether it is formed once or per head), so O, m and s are bit for bit those of the ungrouped _kv8 / _kv8_mx / _kv4_mx
// call on codes and scales repeated g times along the head axis - empty rows, -inf rows, split rows and the NaN of a NaN
// code or scale code 255 included - and DESIGN.md 19's error bound holds unchanged.
//
// Q is always 16 bit: attnQkvGqa's rule, registers while G NL <= 16 and the wave's own LDS region above, read back per
// piece through an opaque offset.  Stores are attnQkvKv's, per head; chunk partials go to attnQkv's workspace layout
// indexed by QUERY head and attnQkvMerge finishes split rows unchanged.
// Templates: MODE, FMT 0 / 1 / 2 = e4m3fn / e5m2 / e2m1, MX (always with e2m1), NL in {1, 2, 4, 8} (K <= 256), G in {4, 8}
// (g = 2 runs in G = 4 with two clamped heads: csrc/attention_qkv_gqa_kv.hip).
// No atomics, one writer per element, every address formed in 64 bits (row and scale strides in bytes), fp contraction
// off, the accurate expf; built without packed fp32 operations like its siblings (csrc/attention_qkv_gqa_kv.hip).
#pragma once

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "attention_qkv_gqa_kernels.hpp"   // qkvGqaQLds (attnQkvGqa itself is not instantiated by this unit)
#include "attention_qkv_kv_kernels.hpp"    // qkvWiden, QkvPiece (attnQkvKv itself is not instantiated by this unit)

namespace bsmr {

// Ks / Vs: the E8M0 scales [b / g][N][K / 32] and [b / g][N][Kv / 32], read only with MX
template <int MODE, int FMT, bool MX, int NL, int G>
__global__ void __launch_bounds__(256)
attnQkvGqaKv(const BwItem* __restrict__ items, uint32_t numItems, const uint32_t* __restrict__ src, float scale,
             const uint16_t* __restrict__ Q, const uint8_t* __restrict__ Kt, const uint8_t* __restrict__ Ks,
             const uint8_t* __restrict__ V, const uint8_t* __restrict__ Vs, uint16_t* __restrict__ O, float* __restrict__ mOut,
             float* __restrict__ sOut, float* __restrict__ partial, float* __restrict__ sPart, float* __restrict__ mPart,
             uint32_t K, uint32_t Kv, uint32_t M, uint32_t N, uint32_t numSlots, uint32_t g, uint32_t subs) {
#pragma clang fp contract(off)
    static_assert(FMT != 2 || MX, "e2m1 always carries block scales");
    static_assert(NL <= 8, "one value chunk and the staged rows of Q cover K, Kv <= 256");
    constexpr bool QLDS = qkvGqaQLds(NL, G);
    constexpr uint32_t qRow = 4u * NL;            // u32x4 per staged row of Q (K / 8 <= 4 NL)
    constexpr uint32_t CB = FMT == 2 ? 4u : 8u;   // code bytes per 8 elements
    constexpr int VE = FMT == 2 ? 8 : 4;          // features per lane: one 32-bit word of codes
    using Piece = typename QkvPiece<FMT>::T;
    __shared__ u32x4 qLds[QLDS ? 4 * G * qRow : 1];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t it = (uint64_t)blockIdx.x * 4u + wave;
    if (it >= numItems) return;   // (whole waves leave: nothing below synchronises across waves)
    const BwItem item = items[it];
    const uint64_t kvHead = blockIdx.y / subs;
    const uint32_t first = (blockIdx.y % subs) * (uint32_t)G;   // the sub-group's first head within its KV group
    const uint32_t quarter = lane & 3u, ent = lane >> 2, kc = K / 32u, vc = Kv / 32u;
    const uint32_t kRow = K / 8u * CB, vRow = Kv / 8u * CB;   // bytes per row of Kt, of V
    const uint32_t len = item.end - item.begin, nt = (len + kQkvTile - 1u) / kQkvTile;
    const bool vOn = 4u * lane < vRow;   // this lane's word of codes lies inside a row of V
    const uint8_t* kb = Kt + kvHead * N * kRow + quarter * CB;
    const uint8_t* ksb = MX ? Ks + kvHead * N * kc : nullptr;
    const uint8_t* vb = V + kvHead * N * vRow + 4u * lane;
    const uint8_t* vsb = MX ? Vs + kvHead * N * vc + (uint32_t)VE * lane / 32u : nullptr;
    uint64_t head[G];   // the query head of h: past the group it repeats the group's last head (wave-uniform, stores nothing)
#pragma unroll
    for (int h = 0; h < G; ++h) head[h] = kvHead * g + min(first + (uint32_t)h, g - 1u);

    u32x4 q[QLDS ? 1 : G][QLDS ? 1 : NL] = {};
    if (nt) {   // (an empty row reads nothing: with nnz = 0 the operands may be NULL)
        if constexpr (QLDS) {
#pragma unroll
            for (int h = 0; h < G; ++h)
                if (lane < K / 8u)
                    qLds[(wave * G + h) * qRow + lane] =
                        *reinterpret_cast<const u32x4*>(Q + (head[h] * M + item.dest) * K + 8u * lane);
            smWaveSync();
        } else {
#pragma unroll
            for (int h = 0; h < G; ++h) {
                const uint16_t* qr = Q + (head[h] * M + item.dest) * K;
#pragma unroll
                for (int i = 0; i < NL; ++i)   // (a piece past K / 32 repeats the last one and is never dotted: no branch)
                    q[h][i] = *reinterpret_cast<const u32x4*>(qr + 32u * min((uint32_t)i, kc - 1u) + 8u * quarter);
            }
        }
    }
    // column ids of the item's entries [64 gr, 64 gr + 64), one per lane
    auto groupCols = [&](uint32_t gr) -> uint32_t {
        const uint32_t e = gr * 64u + lane;
        return e < len ? src[item.begin + e] : 0u;
    };
    // this lane's code pieces of its entry's row of Kt in tile t and their scale codes, read once for the G heads; cols: the
    // ids of the group tile t lies in.  Branch-free as in attnQkvKv: a lane past the item's end reads row 0, a piece past
    // K / 32 repeats the last one; neither is used.
    auto loadKt = [&](uint32_t cols, uint32_t t, Piece (&kt)[NL], uint32_t (&ks)[MX ? NL : 1]) {
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
    // z_h of this lane's entry in tile t for every head, the same bits on the entry's four lanes: attnQkvKv's chain per
    // head, each piece widened once for all of them
    auto score = [&](const Piece (&kt)[NL], const uint32_t (&ks)[MX ? NL : 1], uint32_t t, float (&z)[G]) {
        float p[G];
#pragma unroll
        for (int h = 0; h < G; ++h) p[h] = 0.0f;
        // The staged rows are read again for every tile: the offset is made opaque per call, or the compiler hoists all
        // G NL reads out of the tile loop and the rows live in 4 G NL registers after all.
        uint32_t qAt = wave * G * qRow + quarter;
        if constexpr (QLDS) asm volatile("" : "+v"(qAt));
#pragma unroll
        for (int i = 0; i < NL; ++i) {
            const u32x4 ki = qkvWiden<MODE, FMT>(kt[i]);
            float sc = 1.0f;
            if constexpr (MX) sc = bwScaleMx(ks[i]);
#pragma unroll
            for (int h = 0; h < G; ++h) {
                u32x4 qi;
                if constexpr (QLDS) qi = qLds[qAt + h * qRow + 4u * min((uint32_t)i, kc - 1u)];
                else qi = q[h][i];
                float next;
                if constexpr (MX) next = fmaf(ResidueLowp<MODE>::dot(qi, ki, 0.0f), sc, p[h]);
                else next = ResidueLowp<MODE>::dot(qi, ki, p[h]);
                p[h] = (uint32_t)i < kc ? next : p[h];   // (wave-uniform select: the chain has exactly K / 32 steps)
            }
        }
        const bool inside = t * kQkvTile + ent < len;
#pragma unroll
        for (int h = 0; h < G; ++h) {
            float x = p[h];
            x = x + __shfl_xor(x, 1, 64);
            x = x + __shfl_xor(x, 2, 64);
            z[h] = inside ? scale * x : -INFINITY;
        }
    };
    // the row of V of entry c, read once for the G heads: this lane's word of codes and, with MX, its scale code
    struct VRow {
        uint32_t x, e;
    };
    auto loadV = [&](uint32_t c) -> VRow {
        VRow r;
        r.x = vOn ? *reinterpret_cast<const uint32_t*>(vb + (uint64_t)c * vRow) : 0u;
        r.e = 127u;
        if constexpr (MX) r.e = vOn ? vsb[(uint64_t)c * vc] : 127u;
        return r;
    };
    // the lane's VE elements of a row as fp32, widened and scaled once for the G heads: attnQkvKv's x, bit for bit
    auto widenV = [&](const VRow& r, float (&x)[VE]) {
        if constexpr (FMT == 2) bwWiden4(r.x, x);
        else bwWiden8<FMT>(r.x, x);
        if constexpr (MX) {
            const float sc = bwScaleMx(r.e);
#pragma unroll
            for (int k = 0; k < VE; ++k) x[k] = x[k] * sc;
        }
    };
    float acc[G][VE];
#pragma unroll
    for (int h = 0; h < G; ++h)
#pragma unroll
        for (int k = 0; k < VE; ++k) acc[h][k] = 0.0f;
    auto fmaV = [&](float (&a)[VE], float w, const float (&x)[VE]) {
#pragma unroll
        for (int k = 0; k < VE; ++k) a[k] = fmaf(w, x[k], a[k]);
    };
    auto weight = [](uint32_t e, uint32_t l) -> float { return __uint_as_float(__builtin_amdgcn_readlane(e, l)); };

    float m[G], s[G];
    bool nan[G];
#pragma unroll
    for (int h = 0; h < G; ++h) {
        m[h] = -INFINITY;
        s[h] = 0.0f;
        nan[h] = false;
    }
    if (nt) {
        uint32_t cV = groupCols(0), cK = cV, cNext = groupCols(1);
        Piece kt[NL] = {};
        uint32_t ks[MX ? NL : 1] = {};
        loadKt(cK, 0, kt, ks);
        float z[G];
        score(kt, ks, 0, z);
        for (uint32_t t = 0; t < nt; ++t) {
            const bool more = t + 1u < nt;
            if (more) {   // tile t + 1's rows of Kt fly during tile t's softmax and value phase
                if (((t + 1u) & 3u) == 0) {
                    cK = cNext;
                    cNext = groupCols((t + 1u) / 4u + 1u);
                }
                loadKt(cK, t + 1u, kt, ks);
            }
            uint32_t e[G], live = 0;   // live: bit h set once m_h left -inf (the same on every lane)
#pragma unroll
            for (int h = 0; h < G; ++h) {
                float tm = z[h];
                for (int o = 32; o >= 4; o >>= 1) tm = fmaxf(tm, __shfl_xor(tm, o, 64));   // (the 4 lanes of a quad agree)
                nan[h] |= __any(z[h] != z[h]) != 0;
                const float mNew = smRowMax(fmaxf(m[h], tm), nan[h]);
                if (mNew != m[h]) {   // wave-uniform (a NaN keeps rescaling: the row stays NaN)
                    if (m[h] != -INFINITY) {
                        const float alpha = expf(m[h] - mNew);
                        s[h] = s[h] * alpha;
#pragma unroll
                        for (int k = 0; k < VE; ++k) acc[h][k] = acc[h][k] * alpha;
                    }
                    m[h] = mNew;
                }
                e[h] = __float_as_uint(smExp(z[h], m[h]));
                live |= (m[h] == -INFINITY ? 0u : 1u) << h;
            }
            live = (uint32_t)__builtin_amdgcn_readfirstlane((int)live);
            // While m_h = -inf every e_h so far is 0: head h's value statements of the tile are skipped, so that a non-finite
            // row of V behind a -inf score cannot reach acc_h as 0 * inf.  The rows of V are read when any head is live.
            const uint32_t n = live ? min(kQkvTile, len - t * kQkvTile) : 0u, base = (t & 3u) * kQkvTile;
            uint32_t j = 0;
            for (; j + 4u <= n; j += 4u) {
                const uint32_t c0 = __builtin_amdgcn_readlane(cV, base + j), c1 = __builtin_amdgcn_readlane(cV, base + j + 1u);
                const uint32_t c2 = __builtin_amdgcn_readlane(cV, base + j + 2u), c3 = __builtin_amdgcn_readlane(cV, base + j + 3u);
                const VRow r0 = loadV(c0), r1 = loadV(c1), r2 = loadV(c2), r3 = loadV(c3);
                float x0[VE], x1[VE], x2[VE], x3[VE];
                widenV(r0, x0);
                widenV(r1, x1);
                widenV(r2, x2);
                widenV(r3, x3);
#pragma unroll
                for (int h = 0; h < G; ++h) {
                    if (live >> h & 1u) {
                        const float w0 = weight(e[h], 4u * j), w1 = weight(e[h], 4u * j + 4u);
                        const float w2 = weight(e[h], 4u * j + 8u), w3 = weight(e[h], 4u * j + 12u);
                        s[h] = s[h] + w0;
                        s[h] = s[h] + w1;
                        s[h] = s[h] + w2;
                        s[h] = s[h] + w3;
                        fmaV(acc[h], w0, x0);
                        fmaV(acc[h], w1, x1);
                        fmaV(acc[h], w2, x2);
                        fmaV(acc[h], w3, x3);
                    }
                }
            }
            for (; j < n; ++j) {
                const uint32_t cj = __builtin_amdgcn_readlane(cV, base + j);
                const VRow rj = loadV(cj);
                float xj[VE];
                widenV(rj, xj);
#pragma unroll
                for (int h = 0; h < G; ++h) {
                    if (live >> h & 1u) {
                        const float wj = weight(e[h], 4u * j);
                        s[h] = s[h] + wj;
                        fmaV(acc[h], wj, xj);
                    }
                }
            }
            if (more) score(kt, ks, t + 1u, z);
            if (((t + 1u) & 3u) == 0) cV = cK;
        }
    }
    const uint32_t f0 = (uint32_t)VE * lane;   // this lane's first feature
#pragma unroll
    for (int h = 0; h < G; ++h) {
        if (first + (uint32_t)h >= g) continue;   // a clamped duplicate: its head is stored by the wave that owns it
        if (item.slot == kBwDirect) {   // the one store of a finished row
            const bool dead = m[h] == -INFINITY;   // an empty row, or every score -inf: s = 0
            const uint64_t row = head[h] * M + item.dest;
            if (f0 < Kv) {
                uint32_t w[VE / 2];
#pragma unroll
                for (int k = 0; k < VE / 2; ++k)
                    w[k] = bwNarrow<MODE>(attnDiv(acc[h][2 * k], s[h], dead), attnDiv(acc[h][2 * k + 1], s[h], dead));
                uint16_t* o = O + row * Kv + f0;
                if constexpr (VE == 8) {
                    u32x4 o16 = {w[0], w[1], w[2], w[3]};
                    *reinterpret_cast<u32x4*>(o) = o16;
                } else {
                    u32x2 o16 = {w[0], w[1]};
                    *reinterpret_cast<u32x2*>(o) = o16;
                }
            }
            if (lane == 0) {
                mOut[row] = m[h];
                sOut[row] = s[h];
            }
        } else {
            const uint64_t slot = head[h] * numSlots + item.slot;
            if (f0 < Kv) {
                float* p = partial + slot * Kv + f0;
#pragma unroll
                for (int k = 0; k < VE; k += 4)
                    *reinterpret_cast<float4*>(p + k) = make_float4(acc[h][k], acc[h][k + 1], acc[h][k + 2], acc[h][k + 3]);
            }
            if (lane == 0) {
                mPart[slot] = m[h];
                sPart[slot] = s[h];
            }
        }
    }
}

}  // namespace bsmr
