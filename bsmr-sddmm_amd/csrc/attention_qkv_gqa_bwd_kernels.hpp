// One-pass backward of sparse attention with grouped key/value heads (csrc/attention_qkv_gqa_bwd_capi.hpp,
// bsmr_sparse_attention_qkv_gqa_backward_16; include/bsmr_hip.h "One-pass backward of sparse attention with grouped
// key/value heads"): dQ [b], dKt and dV [b / g] from Q, O, dO, m, s with b query heads and Kt, V with b / g
// key/value heads; query head h reads KV head h / g.  Nothing is repeated in memory and nothing is folded afterwards.
// Per entry the statements are those of csrc/attention_qkv_bwd_kernels.hpp (bwdQuadDot, bwdEntry, bwdAxpy, bwdFinish): the
// same p_t, w_t and dz_t bits on both sides, fp contraction off, the accurate expf.
//
// Column side, attnQkvGqaBwdKV: one wave per column BwItem and KV head, 4 waves per block, grid y = b / g.  The sums dKt_c
// and dV_c belong to the KV head, so the wave loads its own rows Kt_c and V_c once and walks the group's heads 0 ... g - 1
// in ascending order over the item's entries, feeding ONE set of 8 NL + 8 NLV accumulators: slot `ent` is one fmaf chain
// from +0 over the heads ascending and, within a head, over the entries ent, ent + 16, ... ascending (an entry with w = 0
// dropped by the select).  g is a run-time value: the (head, tile) loop is flat, so the prefetch of the next tile crosses
// head boundaries; the 64-entry id groups are read again per head (cache hits).  The item ends as attnQkvBwdKV's does: the
// butterfly over the lane offsets 4, 8, 16, 32, then one rounding (a direct item) or the fp32 partial of a chunk item in
// colPart [b / g][slots][K + Kv], which attnQkvBwdReduce adds in chunk order.  dKt and dV are therefore rounded once from
// an fp32 sum over the whole group.
//
// Row side, attnQkvGqaBwdQ: one wave per row BwItem and sub-group of G consecutive heads of a KV group, as attnQkvGqa; grid
// y = (b / g) ceil(g / G); a sub-group that ends past the group clamps its surplus heads to the group's last head, which
// compute a duplicate and store nothing.  Per tile the column ids and the gathered pieces of Kt_c and V_c are loaded once
// per wave; every head keeps its own rows Q_r and dO_r, its (m, s, D) and its 8 NL accumulators and runs attnQkvBwdQ's
// statements in attnQkvBwdQ's order on them.  Contract: dQ is bit for bit bsmr_sparse_attention_qkv_backward_16's dQ on Kt
// and V repeated g times - direct and split rows; the row partials stay indexed by query head.
// The own rows: with G = 1 they are attnQkvBwdQ's BwdRow; with G > 1 they stay in registers while G (NL + NLV) <= 16 (64
// VGPRs) and are staged in the wave's own LDS region above that (G (K + Kv) 2 bytes), read back per tile through an offset
// the compiler cannot see through - otherwise it hoists the reads out of the tile loop and the rows live in registers
// after all.
// No atomics, one writer per element, every address formed in 64 bits.  Every row of dQ, dKt and dV is written.
#pragma once

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "attention_qkv_bwd_kernels.hpp"   // BwdRow, bwdLoadTile, bwdQuadDot, bwdEntry, bwdAxpy, bwdFinish, bwdTiles, BwdIds
#include "backward_lists.hpp"              // BwItem, kBwDirect
#include "lowp_device.hpp"                 // u32x4
#include "softmax_device.hpp"              // smWaveSync

namespace bsmr {

// ---- the column side: dKt and dV of a KV head, summed over its group ------------------------------------------------
// items / src: the handle's column direction.  Q, dO, m, s, D have kvHeads g heads, Kt, V, dKt, dV and partial kvHeads.
template <int MODE, int NL, int NLV>
__global__ void __launch_bounds__(256)
attnQkvGqaBwdKV(const BwItem* __restrict__ items, uint32_t numItems, const uint32_t* __restrict__ src, float scale,
                const uint16_t* __restrict__ Q, const uint16_t* __restrict__ Kt, const uint16_t* __restrict__ V,
                const uint16_t* __restrict__ dO, const float* __restrict__ mIn, const float* __restrict__ sIn,
                const float* __restrict__ D, uint16_t* __restrict__ dKt, uint16_t* __restrict__ dV,
                float* __restrict__ partial, uint32_t K, uint32_t Kv, uint32_t M, uint32_t N, uint32_t numSlots, uint32_t g) {
#pragma clang fp contract(off)
    constexpr bool kLds = NL > 4 || NLV > 4;
    __shared__ u32x4 lds[kLds ? 4 * 64 : 1];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t it = (uint64_t)blockIdx.x * 4u + wave;
    if (it >= numItems) return;   // (whole waves leave: nothing below synchronises across waves)
    const BwItem item = items[it];
    const uint64_t kvHead = blockIdx.y, col = kvHead * N + item.dest;
    const uint32_t quarter = lane & 3u, ent = lane >> 2, kc = K / 32u, vc = Kv / 32u;
    const uint32_t len = item.end - item.begin, nt = (len + kQkvBwdTile - 1u) / kQkvBwdTile;

    float accK[8 * NL], accV[8 * NLV];
#pragma unroll
    for (int i = 0; i < 8 * NL; ++i) accK[i] = 0.0f;
#pragma unroll
    for (int i = 0; i < 8 * NLV; ++i) accV[i] = 0.0f;
    if (nt) {   // (an empty column reads nothing)
        BwdRow<NL> k = {};
        BwdRow<NLV> v = {};
        u32x4* area = lds + (kLds ? wave * 64u : 0u);
        k.load(Kt + col * K, kc, lane, area);
        v.load(V + col * Kv, vc, lane, area + (kLds ? 32 : 0));
        if constexpr (kLds) smWaveSync();
        const uint64_t head0 = kvHead * g * M;   // the group's first row of Q, dO, m, s, D
        const uint16_t* qb = Q + head0 * K + quarter * 8u;
        const uint16_t* gb = dO + head0 * Kv + quarter * 8u;
        BwdIds ids{src + item.begin, len, lane, 0u, 0u};
        struct Buf {
            BwdTileRows<NL, NLV> x;
            float m, s, d;   // of the entry's row, on the entry's first lane
        };
        // The flat loop over (head, tile): the loads run one step ahead of the arithmetic, each with its own cursor.
        uint32_t lt = 0, ct = 0;   // the tile within the head: of the next load, of the next compute
        uint64_t lrow = 0;         // h M of the next load's head
        bwdTiles<kQkvBwdPingPong<NL, NLV>, Buf>(
            nt * g,
            [&](uint32_t, Buf& y) {
                if (lt == 0) ids.start();   // the head's first tile: the id groups from the start again
                const uint64_t r = lrow + ids.of(lt);
                bwdLoadTile(qb + r * K, kc, y.x.a);
                bwdLoadTile(gb + r * Kv, vc, y.x.b);
                y.m = y.s = y.d = 0.0f;
                if (quarter == 0) {   // one lane per entry
                    y.m = mIn[head0 + r];
                    y.s = sIn[head0 + r];
                    y.d = D[head0 + r];
                }
                if (++lt == nt) {
                    lt = 0;
                    lrow += M;
                }
            },
            [&](uint32_t, const Buf& y) {
                const float p = bwdQuadDot<MODE, false>(k, y.x.a, kc, quarter);
                const float dW = bwdQuadDot<MODE, false>(v, y.x.b, vc, quarter);
                const int first = (int)(lane & ~3u);
                const float m = __shfl(y.m, first, 64), s = __shfl(y.s, first, 64), d = __shfl(y.d, first, 64);
                const BwdEntry e = bwdEntry(p, dW, scale, m, s, d, ct * kQkvBwdTile + ent < len);
                if (e.keep) {
                    bwdAxpy<MODE>(e.dz, y.x.a, kc, accK);
                    bwdAxpy<MODE>(e.w, y.x.b, vc, accV);
                }
                if (++ct == nt) ct = 0;
            });
    }
    if (item.slot == kBwDirect) {
        if (dKt) bwdFinish<MODE, NL>(accK, kc, lane, dKt + col * K, nullptr);
        if (dV) bwdFinish<MODE, NLV>(accV, vc, lane, dV + col * Kv, nullptr);
    } else {
        float* part = partial + (kvHead * numSlots + item.slot) * ((uint64_t)K + Kv);
        bwdFinish<MODE, NL>(accK, kc, lane, nullptr, part);
        bwdFinish<MODE, NLV>(accV, vc, lane, nullptr, part + K);
    }
}

// ---- the row side: dQ of G heads of a KV group -------------------------------------------------------------------------
// whether attnQkvGqaBwdQ<., NL, NLV, G> stages its own rows in LDS (G = 1 keeps attnQkvBwdQ's BwdRow)
constexpr bool qkvGqaBwdOwnLds(int NL, int NLV, int G) { return G > 1 && G * (NL + NLV) > 16; }

// An own row staged in LDS, as bwdQuadDot reads it: at - the row's first u32x4 plus the lane's quarter
struct GqaBwdLdsRow {
    const u32x4* at;
    __device__ __forceinline__ u32x4 piece(int i, uint32_t pc, uint32_t) const { return at[4u * min((uint32_t)i, pc - 1u)]; }
};

// items / src: the handle's row direction.  subs: the sub-groups of a KV group, ceil(g / G).
template <int MODE, int NL, int NLV, int G>
__global__ void __launch_bounds__(256)
attnQkvGqaBwdQ(const BwItem* __restrict__ items, uint32_t numItems, const uint32_t* __restrict__ src, float scale,
               const uint16_t* __restrict__ Q, const uint16_t* __restrict__ Kt, const uint16_t* __restrict__ V,
               const uint16_t* __restrict__ dO, const float* __restrict__ mIn, const float* __restrict__ sIn,
               const float* __restrict__ D, uint16_t* __restrict__ dQ, float* __restrict__ partial, uint32_t K, uint32_t Kv,
               uint32_t M, uint32_t N, uint32_t numSlots, uint32_t g, uint32_t subs) {
#pragma clang fp contract(off)
    constexpr bool OWN = qkvGqaBwdOwnLds(NL, NLV, G);
    constexpr bool kLds = G == 1 && (NL > 4 || NLV > 4);   // BwdRow's own staging
    constexpr uint32_t kRow = 4u * (NL + NLV);             // u32x4 per staged head: Q_r (K / 8 <= 4 NL), then dO_r
    __shared__ u32x4 lds[OWN ? 4 * G * kRow : kLds ? 4 * 64 : 1];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t it = (uint64_t)blockIdx.x * 4u + wave;
    if (it >= numItems) return;   // (whole waves leave: nothing below synchronises across waves)
    const BwItem item = items[it];
    const uint64_t kvHead = blockIdx.y / subs;
    const uint32_t first = (blockIdx.y % subs) * (uint32_t)G;   // the sub-group's first head within its KV group
    const uint32_t quarter = lane & 3u, ent = lane >> 2, kc = K / 32u, vc = Kv / 32u;
    const uint32_t len = item.end - item.begin, nt = (len + kQkvBwdTile - 1u) / kQkvBwdTile;
    uint64_t head[G], row[G];   // the query head of h - past the group it repeats the group's last head - and its row
#pragma unroll
    for (int h = 0; h < G; ++h) {
        head[h] = kvHead * g + min(first + (uint32_t)h, g - 1u);
        row[h] = head[h] * M + item.dest;
    }

    float acc[G][8 * NL];
#pragma unroll
    for (int h = 0; h < G; ++h)
#pragma unroll
        for (int i = 0; i < 8 * NL; ++i) acc[h][i] = 0.0f;
    if (nt) {   // (an empty row reads nothing: with nnz = 0 the operands may be NULL)
        BwdRow<NL> q[OWN ? 1 : G] = {};
        BwdRow<NLV> go[OWN ? 1 : G] = {};
        float m[G], s[G], d[G];
#pragma unroll
        for (int h = 0; h < G; ++h) {
            if constexpr (OWN) {
                u32x4* area = lds + (wave * G + h) * kRow;
                if (lane < K / 8u) area[lane] = *reinterpret_cast<const u32x4*>(Q + row[h] * K + 8u * lane);
                if (lane < Kv / 8u) area[4 * NL + lane] = *reinterpret_cast<const u32x4*>(dO + row[h] * Kv + 8u * lane);
            } else {
                u32x4* area = lds + (kLds ? wave * 64u : 0u);
                q[h].load(Q + row[h] * K, kc, lane, area);
                go[h].load(dO + row[h] * Kv, vc, lane, area + (kLds ? 32 : 0));
            }
            m[h] = mIn[row[h]];
            s[h] = sIn[row[h]];
            d[h] = D[row[h]];
        }
        if constexpr (OWN || kLds) smWaveSync();
        const uint16_t* kb = Kt + kvHead * N * K + quarter * 8u;
        const uint16_t* vb = V + kvHead * N * Kv + quarter * 8u;
        BwdIds ids{src + item.begin, len, lane, 0u, 0u};
        ids.start();
        using Buf = BwdTileRows<NL, NLV>;
        bwdTiles<kQkvBwdPingPong<NL, NLV>, Buf>(
            nt,
            [&](uint32_t t, Buf& x) {   // the tile's rows of Kt and V, once for the G heads
                const uint64_t c = ids.of(t);
                bwdLoadTile(kb + c * K, kc, x.a);
                bwdLoadTile(vb + c * Kv, vc, x.b);
            },
            [&](uint32_t t, const Buf& x) {
                const bool live = t * kQkvBwdTile + ent < len;
                uint32_t at = wave * G * kRow + quarter;
                if constexpr (OWN) asm volatile("" : "+v"(at));   // opaque per tile: the staged rows are read again
#pragma unroll
                for (int h = 0; h < G; ++h) {
                    float p, dW;
                    if constexpr (OWN) {
                        p = bwdQuadDot<MODE, true, NL>(GqaBwdLdsRow{lds + at + h * kRow}, x.a, kc, quarter);
                        dW = bwdQuadDot<MODE, true, NLV>(GqaBwdLdsRow{lds + at + h * kRow + 4 * NL}, x.b, vc, quarter);
                    } else {
                        p = bwdQuadDot<MODE, true, NL>(q[h], x.a, kc, quarter);
                        dW = bwdQuadDot<MODE, true, NLV>(go[h], x.b, vc, quarter);
                    }
                    const BwdEntry e = bwdEntry(p, dW, scale, m[h], s[h], d[h], live);
                    if (e.keep) bwdAxpy<MODE>(e.dz, x.a, kc, acc[h]);
                }
            });
    }
    const bool direct = item.slot == kBwDirect;
#pragma unroll
    for (int h = 0; h < G; ++h) {
        if (first + (uint32_t)h >= g) continue;   // a clamped duplicate (wave-uniform): its head is stored by its own wave
        bwdFinish<MODE, NL>(acc[h], kc, lane, direct ? dQ + row[h] * K : nullptr,
                            direct ? nullptr : partial + (head[h] * numSlots + item.slot) * K);
    }
}

}  // namespace bsmr
