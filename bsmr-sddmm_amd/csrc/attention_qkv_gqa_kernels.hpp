// One-pass sparse attention with grouped key/value heads (csrc/attention_qkv_gqa_capi.hpp, bsmr_sparse_attention_qkv_gqa_16;
// include/bsmr_hip.h "One-pass sparse attention with grouped key/value heads"): b query heads read b / g
// key/value heads, query head h reads KV head h / g (the repeat_interleave convention).  S is shared by all heads, so the g
// heads of a KV group walk the same entries in the same order: a wave that serves several of them gathers each row of Kt
// and of V and each column id once.
//
// attnQkvGqa runs one wave per BwItem and sub-group of a KV group, 4 waves per block (4 items, one sub-group); grid y =
// (b / g) * ceil(g / G) sub-groups.  A sub-group is G consecutive heads of a group; one that ends past the group (g = 3, 7,
// ...) clamps its surplus head indices to the group's last head: those heads compute a duplicate and store nothing.
//
// Per tile of kQkvTile = 16 entries the wave loads the column ids, the Kt tile (loadKt: attnQkv's score layout, NL pieces
// per lane) and each entry's row of V (loadV: attnQkv's value layout, 4 rows in flight) ONCE, and every head h < G keeps its
// own p_h, z_h, (m_h, s_h, nan_h), e_h and acc_h[2 VC] and runs attnQkv's statements on them in attnQkv's order: the dot
// chain over the pieces in ascending i, the two quad steps, fl(scale p), the tile maximum, the rescale by expf(fl(m - m')),
// smExp, s += e and fmaf(e, V, acc) in entry order.  A row of V feeds G fmaV calls, each with its weight read from e_h by
// v_readlane.  The "skip while m = -inf" rule is per head: a head whose m_h is still -inf skips its s / acc statements of
// the tile behind a wave-uniform branch (0 * inf stays out of acc, as in attnQkv); the tile's rows of V are loaded when any
// head of the wave is live.
// Contract: every head runs attnQkv's statement sequence on the same values, so O, m and s are bit for bit those of
// bsmr_sparse_attention_qkv_16 on Kt and V repeated g times along the head axis - empty rows, -inf rows, NaN propagation
// and split rows included - and DESIGN.md 18's error bound holds unchanged.
//
// The G rows of Q: with G NL <= 16 each lane keeps its pieces of all G rows in registers (at most 64 VGPRs); above that
// the rows are staged in the wave's own LDS region (G K 2 bytes, 4 KiB at K = 256, G = 8) and read back per piece.
// Stores are attnQkv's, per head: a direct item divides, rounds once and stores O, m, s; a chunk item writes (m_c, s_c,
// acc_c) to attnQkv's workspace layout [b][slots] indexed by QUERY head, and attnQkvMerge finishes split rows unchanged.
// Templates: MODE, NL (1, 2, 4, 8: K <= 256), VC (1, 2: Kv <= 256) as attnQkv's; G in {2, 4, 8}.
// No atomics, one writer per element, every address formed in 64 bits, fp contraction off, the accurate expf; built
// without packed fp32 operations like its siblings (csrc/attention_qkv_gqa.hip).
#pragma once

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "attention_qkv_kernels.hpp"   // kQkvTile (attnQkv itself is not instantiated by this unit)
#include "backward_lists.hpp"          // BwItem, kBwDirect
#include "lowp_device.hpp"             // u32x4, ResidueLowp, bwWiden, bwNarrow
#include "softmax_device.hpp"          // attnDiv, smExp, smRowMax, smWaveSync

namespace bsmr {

// whether attnQkvGqa<., NL, ., G> stages its rows of Q in LDS
constexpr bool qkvGqaQLds(int NL, int G) { return G * NL > 16; }

template <int MODE, int NL, int VC, int G>
__global__ void __launch_bounds__(256)
attnQkvGqa(const BwItem* __restrict__ items, uint32_t numItems, const uint32_t* __restrict__ src, float scale,
           const uint16_t* __restrict__ Q, const uint16_t* __restrict__ Kt, const uint16_t* __restrict__ V,
           uint16_t* __restrict__ O, float* __restrict__ mOut, float* __restrict__ sOut, float* __restrict__ partial,
           float* __restrict__ sPart, float* __restrict__ mPart, uint32_t K, uint32_t Kv, uint32_t M, uint32_t N,
           uint32_t numSlots, uint32_t g, uint32_t subs) {
#pragma clang fp contract(off)
    constexpr bool QLDS = qkvGqaQLds(NL, G);
    constexpr uint32_t kRow = 4u * NL;   // u32x4 per staged row of Q (K / 8 <= 4 NL)
    __shared__ u32x4 qLds[QLDS ? 4 * G * kRow : 1];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t it = (uint64_t)blockIdx.x * 4u + wave;
    if (it >= numItems) return;   // (whole waves leave: nothing below synchronises across waves)
    const BwItem item = items[it];
    const uint64_t kvHead = blockIdx.y / subs;
    const uint32_t first = (blockIdx.y % subs) * (uint32_t)G;   // the sub-group's first head within its KV group
    const uint32_t quarter = lane & 3u, ent = lane >> 2, kc = K / 32u, pairs = Kv / 2u;
    const uint32_t len = item.end - item.begin, nt = (len + kQkvTile - 1u) / kQkvTile;
    const uint16_t* kb = Kt + kvHead * N * K + quarter * 8u;
    const uint16_t* vb = V + kvHead * N * Kv + 2u * lane;
    uint64_t head[G];   // the query head of h: past the group it repeats the group's last head (wave-uniform, stores nothing)
#pragma unroll
    for (int h = 0; h < G; ++h) head[h] = kvHead * g + min(first + (uint32_t)h, g - 1u);

    u32x4 q[QLDS ? 1 : G][QLDS ? 1 : NL] = {};
    if (nt) {   // (an empty row reads nothing: with nnz = 0 the operands may be NULL)
        if constexpr (QLDS) {
#pragma unroll
            for (int h = 0; h < G; ++h)
                if (lane < K / 8u)
                    qLds[(wave * G + h) * kRow + lane] =
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
    // this lane's pieces of its entry's row of Kt in tile t, read once for the G heads; cols: the ids of the group tile t
    // lies in.  Branch-free as in attnQkv: a lane past the item's end reads row 0, a piece past K / 32 repeats the last one.
    auto loadKt = [&](uint32_t cols, uint32_t t, u32x4 (&kt)[NL]) {
        const uint32_t c = (uint32_t)__shfl((int)cols, (int)((t & 3u) * kQkvTile + ent), 64);
        const uint16_t* row = kb + (uint64_t)c * K;
#pragma unroll
        for (int i = 0; i < NL; ++i) kt[i] = *reinterpret_cast<const u32x4*>(row + 32u * min((uint32_t)i, kc - 1u));
    };
    // z_h of this lane's entry in tile t for every head, the same bits on the entry's four lanes: attnQkv's chain per head
    auto score = [&](const u32x4 (&kt)[NL], uint32_t t, float (&z)[G]) {
        float p[G];
#pragma unroll
        for (int h = 0; h < G; ++h) p[h] = 0.0f;
        // The staged rows are read again for every tile: the offset is made opaque per call, or the compiler hoists all
        // G NL reads out of the tile loop and the rows live in 4 G NL registers after all.
        uint32_t qAt = wave * G * kRow + quarter;
        if constexpr (QLDS) asm volatile("" : "+v"(qAt));
#pragma unroll
        for (int i = 0; i < NL; ++i) {
#pragma unroll
            for (int h = 0; h < G; ++h) {
                u32x4 qi;
                if constexpr (QLDS) qi = qLds[qAt + h * kRow + 4u * min((uint32_t)i, kc - 1u)];
                else qi = q[h][i];
                const float next = ResidueLowp<MODE>::dot(qi, kt[i], p[h]);
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
    // the row of V of entry c, read once for the G heads
    auto loadV = [&](uint32_t c, uint32_t (&x)[VC]) {
        const uint16_t* row = vb + (uint64_t)c * Kv;
#pragma unroll
        for (int i = 0; i < VC; ++i) x[i] = lane + 64u * i < pairs ? *reinterpret_cast<const uint32_t*>(row + 128u * i) : 0u;
    };
    float acc[G][2 * VC];
#pragma unroll
    for (int h = 0; h < G; ++h)
#pragma unroll
        for (int i = 0; i < 2 * VC; ++i) acc[h][i] = 0.0f;
    auto fmaV = [&](float (&a)[2 * VC], float w, const uint32_t (&x)[VC]) {
#pragma unroll
        for (int i = 0; i < VC; ++i) {
            float lo, hi;
            bwWiden<MODE>(x[i], lo, hi);
            a[2 * i] = fmaf(w, lo, a[2 * i]);
            a[2 * i + 1] = fmaf(w, hi, a[2 * i + 1]);
        }
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
        u32x4 kt[NL] = {};
        loadKt(cK, 0, kt);
        float z[G];
        score(kt, 0, z);
        for (uint32_t t = 0; t < nt; ++t) {
            const bool more = t + 1u < nt;
            if (more) {   // tile t + 1's rows of Kt fly during tile t's softmax and value phase
                if (((t + 1u) & 3u) == 0) {
                    cK = cNext;
                    cNext = groupCols((t + 1u) / 4u + 1u);
                }
                loadKt(cK, t + 1u, kt);
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
                        for (int i = 0; i < 2 * VC; ++i) acc[h][i] = acc[h][i] * alpha;
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
                uint32_t x0[VC], x1[VC], x2[VC], x3[VC];
                loadV(c0, x0);
                loadV(c1, x1);
                loadV(c2, x2);
                loadV(c3, x3);
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
                uint32_t xj[VC];
                loadV(cj, xj);
#pragma unroll
                for (int h = 0; h < G; ++h) {
                    if (live >> h & 1u) {
                        const float wj = weight(e[h], 4u * j);
                        s[h] = s[h] + wj;
                        fmaV(acc[h], wj, xj);
                    }
                }
            }
            if (more) score(kt, t + 1u, z);
            if (((t + 1u) & 3u) == 0) cV = cK;
        }
    }
#pragma unroll
    for (int h = 0; h < G; ++h) {
        if (first + (uint32_t)h >= g) continue;   // a clamped duplicate: its head is stored by the wave that owns it
        if (item.slot == kBwDirect) {   // the one store of a finished row
            const bool dead = m[h] == -INFINITY;   // an empty row, or every score -inf: s = 0
            const uint64_t row = head[h] * M + item.dest;
            uint16_t* o = O + row * Kv + 2u * lane;
#pragma unroll
            for (int i = 0; i < VC; ++i)
                if (lane + 64u * i < pairs)
                    *reinterpret_cast<uint32_t*>(o + 128u * i) =
                        bwNarrow<MODE>(attnDiv(acc[h][2 * i], s[h], dead), attnDiv(acc[h][2 * i + 1], s[h], dead));
            if (lane == 0) {
                mOut[row] = m[h];
                sOut[row] = s[h];
            }
        } else {
            const uint64_t slot = head[h] * numSlots + item.slot;
            float* p = partial + slot * Kv + 2u * lane;
#pragma unroll
            for (int i = 0; i < VC; ++i)
                if (lane + 64u * i < pairs)
                    *reinterpret_cast<float2*>(p + 128u * i) = make_float2(acc[h][2 * i], acc[h][2 * i + 1]);
            if (lane == 0) {
                mPart[slot] = m[h];
                sPart[slot] = s[h];
            }
        }
    }
}

}  // namespace bsmr
