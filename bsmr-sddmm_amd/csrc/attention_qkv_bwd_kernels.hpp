// One-pass backward of sparse attention (csrc/attention_qkv_bwd_capi.hpp, bsmr_sparse_attention_qkv_backward_16;
// include/bsmr_hip.h "One-pass backward of sparse attention"): dQ, dKt and dV from Q, Kt, V, O, dO and the
// forward's (m, s).  Scores and weights live in registers only: nothing of size nnz is allocated, written or read.
//
// Contract, per entry t = (r, c) of S; every step is one IEEE fp32 operation, fp contraction off, the accurate expf:
//   p_t  = Q_r . Kt_c exactly as attnQkv's score layout forms it (csrc/attention_qkv_kernels.hpp): lane quarter j runs ONE
//          fp32 accumulator from +0 over the elements 32 i + 8 j ... + 7, i ascending, two elements per dot2<MODE> step with
//          Q's piece as the first operand; then the two quad additions x + lane^1, x + lane^2.
//   z_t  = fl(scale p_t);  e_t = expf(fl(z_t - m_r));  w_t = fl(e_t / s_r), and 0 when m_r = -inf.
//   dW_t = dO_r . V_c in the same quarter layout over Kv (dO's piece first);  D_r = dO_r . O_r from attnRowDot<MODE> on
//          the saved, rounded O (csrc/attention_kernels.hpp: its order is unchanged).
//   dz_t = fl(fl(w_t fl(dW_t - D_r)) scale).
//   dQ_r = sum_t dz_t Kt_c;  dKt_c = sum_t dz_t Q_r;  dV_c = sum_t w_t dO_r, each term one fmaf into the sum.
// Both kernels form p_t from the same operands in the same order as attnQkv, so the row side, the column side and the
// forward see the same bits of z_t, and with the saved (m, s) the same bits of w_t.
// An entry whose w_t is exactly 0 - a dead row, a -inf score, an underflown weight - is dropped by a select, not
// multiplied: a non-finite row behind it reaches no sum (attnQkv skips a tile in the same way while m = -inf).  A NaN in
// row r of Q or dO makes w or dz NaN for the entries of row r alone: it reaches dQ_r and the dKt / dV rows of the columns
// row r stores, and no other row.
//
// Layout.  One wave per BwItem (a row or column of S, or one chunk of a list longer than BSMR_BACKWARD_CHUNK), 4 waves per
// block, batches in grid y.  The item's entries go in tiles of 16 in attnQkv's score layout: lane l serves entry l >> 2,
// quarter l & 3; piece i of a row is the 16 bytes at element 32 i + 8 (l & 3).  The ids of 64 entries come from one
// coalesced load, the next group already in flight.  The item's own rows (Q_r and dO_r on the row side, Kt_c and V_c on
// the column side) stay with the wave: as pieces in registers up to 128 features, beyond that in the wave's 1 KiB of
// LDS.  The gathered rows of a tile are loaded branch-free over the class (NL, NLV in {1, 2, 4, 8} pieces; a piece past
// K / 32 repeats the last one and its dot step is dropped by a wave-uniform select), and the loads of tile t + 1 are
// issued before the arithmetic of tile t (two register buffers, ping-pong) - except in the classes with NL + NLV > 8,
// which keep one buffer so that no instantiation needs scratch.
//
// Summation order - on purpose not bsmr_spmm's sequential chain.  The sums are kept where the data already lies: a lane
// holds 8 NL (8 NLV) fp32 accumulators for the elements of its own quarter and feeds them from the registers that just
// served the dot; nothing is read twice and nothing is broadcast.  Accumulator slot `ent` of an item is the fmaf chain
// from +0 over the entries ent, ent + 16, ent + 32, ... of the item in ascending order (dropped entries left out).  At the
// item's end the 16 slots are added by a butterfly x = x + partner over the lane offsets 4, 8, 16, 32 in this order (fp32
// addition commutes: all lanes end equal); lanes 0 - 3 store.  A direct item rounds once (bwNarrow) and stores 16 bits; a
// chunk item stores its fp32 partial, and attnQkvBwdReduce adds a destination's partials in chunk order, then rounds.
// No atomics, one writer per element, every address formed in 64 bits.  Every row of dQ, dKt and dV is written: a row or
// column without entries gets +0.
#pragma once

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "backward_lists.hpp"   // BwItem, BwSplit, kBwDirect
#include "lowp_device.hpp"      // u32x2, u32x4, ResidueLowp, bwWiden, bwNarrow
#include "softmax_device.hpp"   // smExp, smWaveSync

namespace bsmr {

constexpr uint32_t kQkvBwdTile = 16;   // entries per tile: 64 lanes = 16 entries x 4 quarters of a row

// Whether the class (NL, NLV) prefetches tile t + 1 into a second register buffer
template <int NL, int NLV>
constexpr bool kQkvBwdPingPong = NL + NLV <= 8;

// A row that stays with the wave for the whole item, as this lane's pieces: NP <= 4 in registers, wider in LDS
template <int NP>
struct BwdRow {
    static constexpr bool LDS = NP > 4;
    u32x4 reg[LDS ? 1 : NP];
    const u32x4* lds;
    // row: the row's first element; pc: its pieces (features / 32); area: 32 u32x4 of the wave's own LDS
    __device__ __forceinline__ void load(const uint16_t* row, uint32_t pc, uint32_t lane, u32x4* area) {
        lds = area;
        if constexpr (LDS) {
            if (lane < 4u * pc) area[lane] = *reinterpret_cast<const u32x4*>(row + 8u * lane);
        } else {
#pragma unroll
            for (int i = 0; i < NP; ++i)   // (a piece past pc repeats the last one and is never used: no branch)
                reg[i] = *reinterpret_cast<const u32x4*>(row + 32u * min((uint32_t)i, pc - 1u) + 8u * (lane & 3u));
        }
    }
    __device__ __forceinline__ u32x4 piece(int i, uint32_t pc, uint32_t quarter) const {
        if constexpr (LDS) return lds[4u * min((uint32_t)i, pc - 1u) + quarter];
        else return reg[i];
    }
};

// This lane's pieces of a gathered row (row: already at the lane's quarter); branch-free, so the NP loads fly together
template <int NP>
__device__ __forceinline__ void bwdLoadTile(const uint16_t* row, uint32_t pc, u32x4 (&x)[NP]) {
#pragma unroll
    for (int i = 0; i < NP; ++i) x[i] = *reinterpret_cast<const u32x4*>(row + 32u * min((uint32_t)i, pc - 1u));
}

// The dot of the item's row with this lane's entry's row, the same bits on the entry's four lanes.  FIRST: the item's
// row is the first operand of dot2 (the row side: Q_r, dO_r), otherwise the gathered one is (the column side).  Own: a
// BwdRow<NP>, or any row with its piece(i, pc, quarter).
template <int MODE, bool FIRST, int NP, typename Own>
__device__ __forceinline__ float bwdQuadDot(const Own& own, const u32x4 (&x)[NP], uint32_t pc, uint32_t quarter) {
#pragma clang fp contract(off)
    float p = 0.0f;
#pragma unroll
    for (int i = 0; i < NP; ++i) {
        const u32x4 o = own.piece(i, pc, quarter);
        const float next = FIRST ? ResidueLowp<MODE>::dot(o, x[i], p) : ResidueLowp<MODE>::dot(x[i], o, p);
        p = (uint32_t)i < pc ? next : p;   // (wave-uniform select: the chain has exactly pc steps)
    }
    p = p + __shfl_xor(p, 1, 64);
    p = p + __shfl_xor(p, 2, 64);
    return p;
}

// w_t and dz_t of one entry; live: the lane's entry lies inside the item
struct BwdEntry {
    float w, dz;
    bool keep;   // w != 0 (a NaN is kept)
};
__device__ __forceinline__ BwdEntry bwdEntry(float p, float dW, float scale, float m, float s, float D, bool live) {
#pragma clang fp contract(off)
    BwdEntry e;
    const float ex = smExp(scale * p, m);
    e.w = !live || m == -INFINITY ? 0.0f : ex / s;
    e.dz = (e.w * (dW - D)) * scale;
    e.keep = e.w != 0.0f;
    return e;
}

// acc += a x over this lane's pieces of a row
template <int MODE, int NP>
__device__ __forceinline__ void bwdAxpy(float a, const u32x4 (&x)[NP], uint32_t pc, float (&acc)[8 * NP]) {
#pragma unroll
    for (int i = 0; i < NP; ++i) {
        if ((uint32_t)i >= pc) break;   // wave-uniform
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float lo, hi;
            bwWiden<MODE>(x[i][j], lo, hi);
            acc[8 * i + 2 * j] = fmaf(a, lo, acc[8 * i + 2 * j]);
            acc[8 * i + 2 * j + 1] = fmaf(a, hi, acc[8 * i + 2 * j + 1]);
        }
    }
}

// The end of an item: the 16 entry slots of every accumulator are added over the lane offsets 4, 8, 16, 32, then lanes
// 0 - 3 store their quarter - rounded to out16 (a direct item) or as fp32 to part (a chunk item); both at the row's start.
template <int MODE, int NP>
__device__ __forceinline__ void bwdFinish(float (&acc)[8 * NP], uint32_t pc, uint32_t lane, uint16_t* out16, float* part) {
#pragma clang fp contract(off)
#pragma unroll
    for (int i = 0; i < NP; ++i) {
        if ((uint32_t)i >= pc) break;   // wave-uniform
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            float x = acc[8 * i + k];
            x = x + __shfl_xor(x, 4, 64);
            x = x + __shfl_xor(x, 8, 64);
            x = x + __shfl_xor(x, 16, 64);
            x = x + __shfl_xor(x, 32, 64);
            acc[8 * i + k] = x;
        }
        if (lane < 4u) {
            const uint32_t at = 32u * i + 8u * lane;
            if (out16) {
                u32x4 o;
#pragma unroll
                for (int j = 0; j < 4; ++j) o[j] = bwNarrow<MODE>(acc[8 * i + 2 * j], acc[8 * i + 2 * j + 1]);
                *reinterpret_cast<u32x4*>(out16 + at) = o;
            } else {
                *reinterpret_cast<float4*>(part + at) = make_float4(acc[8 * i], acc[8 * i + 1], acc[8 * i + 2], acc[8 * i + 3]);
                *reinterpret_cast<float4*>(part + at + 4u) =
                    make_float4(acc[8 * i + 4], acc[8 * i + 5], acc[8 * i + 6], acc[8 * i + 7]);
            }
        }
    }
}

// The tile loop of both kernels: load(t, buffer) issues tile t's loads, compute(t, buffer) consumes them.  With PING the
// loads of tile t + 1 are issued before the arithmetic of tile t.
template <bool PING, typename Buf, typename Load, typename Compute>
__device__ __forceinline__ void bwdTiles(uint32_t nt, Load&& load, Compute&& compute) {
    if constexpr (PING) {
        Buf a, b;
        load(0u, a);
        for (uint32_t t = 0; t < nt; t += 2u) {
            if (t + 1u < nt) load(t + 1u, b);
            compute(t, a);
            if (t + 1u < nt) {
                if (t + 2u < nt) load(t + 2u, a);
                compute(t + 1u, b);
            }
        }
    } else {
        Buf a;
        for (uint32_t t = 0; t < nt; ++t) {
            load(t, a);
            compute(t, a);
        }
    }
}

// The ids of an item's entries, 64 per coalesced load, the group after the current one already in flight.  Tiles are
// asked for in ascending order, each once.
struct BwdIds {
    const uint32_t* src;   // at the item's first entry
    uint32_t len, lane, cur, next;
    __device__ __forceinline__ uint32_t group(uint32_t g) const {
        const uint32_t e = g * 64u + lane;
        return e < len ? src[e] : 0u;   // (a lane past the item's end reads row 0 and uses nothing of it)
    }
    __device__ __forceinline__ void start() {
        cur = group(0);
        next = group(1);
    }
    // the id of this lane's entry in tile t
    __device__ __forceinline__ uint32_t of(uint32_t t) {
        if (t && (t & 3u) == 0) {
            cur = next;
            next = group(t / 4u + 1u);
        }
        return (uint32_t)__shfl((int)cur, (int)((t & 3u) * kQkvBwdTile + (lane >> 2)), 64);
    }
};

template <int NL, int NLV>
struct BwdTileRows {   // the two gathered rows of a tile, this lane's pieces
    u32x4 a[NL], b[NLV];
};

// ---- the row side: dQ ------------------------------------------------------------------------------------------------
// items / src: the handle's row direction (items[0], colIndices).  m, s, D [b][M].  A direct item stores dQ[dest], a chunk
// item its partial row (partial, [b][numSlots][K]).
template <int MODE, int NL, int NLV>
__global__ void __launch_bounds__(256)
attnQkvBwdQ(const BwItem* __restrict__ items, uint32_t numItems, const uint32_t* __restrict__ src, float scale,
            const uint16_t* __restrict__ Q, const uint16_t* __restrict__ Kt, const uint16_t* __restrict__ V,
            const uint16_t* __restrict__ dO, const float* __restrict__ mIn, const float* __restrict__ sIn,
            const float* __restrict__ D, uint16_t* __restrict__ dQ, float* __restrict__ partial, uint32_t K, uint32_t Kv,
            uint32_t M, uint32_t N, uint32_t numSlots) {
#pragma clang fp contract(off)
    constexpr bool kLds = NL > 4 || NLV > 4;
    __shared__ u32x4 lds[kLds ? 4 * 64 : 1];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t it = (uint64_t)blockIdx.x * 4u + wave;
    if (it >= numItems) return;   // (whole waves leave: nothing below synchronises across waves)
    const BwItem item = items[it];
    const uint64_t b = blockIdx.y, row = b * M + item.dest;
    const uint32_t quarter = lane & 3u, ent = lane >> 2, kc = K / 32u, vc = Kv / 32u;
    const uint32_t len = item.end - item.begin, nt = (len + kQkvBwdTile - 1u) / kQkvBwdTile;

    float acc[8 * NL];
#pragma unroll
    for (int i = 0; i < 8 * NL; ++i) acc[i] = 0.0f;
    if (nt) {   // (an empty row reads nothing: with nnz = 0 the operands may be NULL)
        BwdRow<NL> q = {};
        BwdRow<NLV> g = {};
        u32x4* area = lds + (kLds ? wave * 64u : 0u);
        q.load(Q + row * K, kc, lane, area);
        g.load(dO + row * Kv, vc, lane, area + (kLds ? 32 : 0));
        if constexpr (kLds) smWaveSync();
        const float m = mIn[row], s = sIn[row], d = D[row];
        const uint16_t* kb = Kt + b * N * K + quarter * 8u;
        const uint16_t* vb = V + b * N * Kv + quarter * 8u;
        BwdIds ids{src + item.begin, len, lane, 0u, 0u};
        ids.start();
        using Buf = BwdTileRows<NL, NLV>;
        bwdTiles<kQkvBwdPingPong<NL, NLV>, Buf>(
            nt,
            [&](uint32_t t, Buf& x) {
                const uint64_t c = ids.of(t);
                bwdLoadTile(kb + c * K, kc, x.a);
                bwdLoadTile(vb + c * Kv, vc, x.b);
            },
            [&](uint32_t t, const Buf& x) {
                const float p = bwdQuadDot<MODE, true>(q, x.a, kc, quarter);
                const float dW = bwdQuadDot<MODE, true>(g, x.b, vc, quarter);
                const BwdEntry e = bwdEntry(p, dW, scale, m, s, d, t * kQkvBwdTile + ent < len);
                if (e.keep) bwdAxpy<MODE>(e.dz, x.a, kc, acc);
            });
    }
    const bool direct = item.slot == kBwDirect;
    bwdFinish<MODE, NL>(acc, kc, lane, direct ? dQ + row * K : nullptr,
                        direct ? nullptr : partial + (b * numSlots + item.slot) * K);
}

// ---- the column side: dKt and dV -----------------------------------------------------------------------------------
// items / src: the handle's column direction (items[1], cscRows: within a column the rows ascend).  A direct item stores
// dKt[dest] and dV[dest] (each unless NULL), a chunk item its partial row (partial, [b][numSlots][K + Kv]: dKt, then dV).
template <int MODE, int NL, int NLV>
__global__ void __launch_bounds__(256)
attnQkvBwdKV(const BwItem* __restrict__ items, uint32_t numItems, const uint32_t* __restrict__ src, float scale,
             const uint16_t* __restrict__ Q, const uint16_t* __restrict__ Kt, const uint16_t* __restrict__ V,
             const uint16_t* __restrict__ dO, const float* __restrict__ mIn, const float* __restrict__ sIn,
             const float* __restrict__ D, uint16_t* __restrict__ dKt, uint16_t* __restrict__ dV,
             float* __restrict__ partial, uint32_t K, uint32_t Kv, uint32_t M, uint32_t N, uint32_t numSlots) {
#pragma clang fp contract(off)
    constexpr bool kLds = NL > 4 || NLV > 4;
    __shared__ u32x4 lds[kLds ? 4 * 64 : 1];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t it = (uint64_t)blockIdx.x * 4u + wave;
    if (it >= numItems) return;   // (whole waves leave: nothing below synchronises across waves)
    const BwItem item = items[it];
    const uint64_t b = blockIdx.y, col = b * N + item.dest;
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
        const uint16_t* qb = Q + b * M * K + quarter * 8u;
        const uint16_t* gb = dO + b * M * Kv + quarter * 8u;
        const float* mb = mIn + b * M;
        const float* sb = sIn + b * M;
        const float* db = D + b * M;
        BwdIds ids{src + item.begin, len, lane, 0u, 0u};
        ids.start();
        struct Buf {
            BwdTileRows<NL, NLV> x;
            float m, s, d;   // of the entry's row, on the entry's first lane
        };
        bwdTiles<kQkvBwdPingPong<NL, NLV>, Buf>(
            nt,
            [&](uint32_t t, Buf& y) {
                const uint64_t r = ids.of(t);
                bwdLoadTile(qb + r * K, kc, y.x.a);
                bwdLoadTile(gb + r * Kv, vc, y.x.b);
                y.m = y.s = y.d = 0.0f;
                if (quarter == 0) {   // one lane per entry
                    y.m = mb[r];
                    y.s = sb[r];
                    y.d = db[r];
                }
            },
            [&](uint32_t t, const Buf& y) {
                const float p = bwdQuadDot<MODE, false>(k, y.x.a, kc, quarter);
                const float dW = bwdQuadDot<MODE, false>(v, y.x.b, vc, quarter);
                const int first = (int)(lane & ~3u);
                const float m = __shfl(y.m, first, 64), s = __shfl(y.s, first, 64), d = __shfl(y.d, first, 64);
                const BwdEntry e = bwdEntry(p, dW, scale, m, s, d, t * kQkvBwdTile + ent < len);
                if (e.keep) {
                    bwdAxpy<MODE>(e.dz, y.x.a, kc, accK);
                    bwdAxpy<MODE>(e.w, y.x.b, vc, accV);
                }
            });
    }
    if (item.slot == kBwDirect) {
        if (dKt) bwdFinish<MODE, NL>(accK, kc, lane, dKt + col * K, nullptr);
        if (dV) bwdFinish<MODE, NLV>(accV, vc, lane, dV + col * Kv, nullptr);
    } else {
        float* part = partial + (b * numSlots + item.slot) * ((uint64_t)K + Kv);
        bwdFinish<MODE, NL>(accK, kc, lane, nullptr, part);
        bwdFinish<MODE, NLV>(accV, vc, lane, nullptr, part + K);
    }
}

// A split destination: its fp32 partials added in chunk order, rounded once, 16 bits stored; one thread per 4 features,
// as attnQkvMerge.  A slot's row is `stride` floats, the gradient's `width` floats lie at `offset` in it; rows: the rows
// of out per batch.
template <int MODE>
__global__ void __launch_bounds__(256)
attnQkvBwdReduce(const BwSplit* __restrict__ splits, uint32_t numSplits, const float* __restrict__ partial, uint32_t stride,
                 uint32_t offset, uint16_t* __restrict__ out, uint32_t width, uint32_t rows, uint32_t numSlots) {
#pragma clang fp contract(off)
    const uint32_t q = width / 4u;
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= (uint64_t)numSplits * q) return;
    const BwSplit sp = splits[i / q];
    const uint64_t c = (i % q) * 4u, b = blockIdx.y;
    const float* pp = partial + (b * numSlots + sp.firstSlot) * stride + offset + c;
    float4 acc = *reinterpret_cast<const float4*>(pp);
    for (uint32_t k = 1; k < sp.numSlots; ++k) {
        const float4 x = *reinterpret_cast<const float4*>(pp + (uint64_t)k * stride);
        acc.x = acc.x + x.x;
        acc.y = acc.y + x.y;
        acc.z = acc.z + x.z;
        acc.w = acc.w + x.w;
    }
    u32x2 o;
    o[0] = bwNarrow<MODE>(acc.x, acc.y);
    o[1] = bwNarrow<MODE>(acc.z, acc.w);
    *reinterpret_cast<u32x2*>(out + (b * rows + sp.dest) * width + c) = o;
}

}  // namespace bsmr
