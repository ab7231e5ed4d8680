// One-pass sparse attention with grouped key/value heads, both products on the MFMA (csrc/attention_qkv_gqa_mfma_capi.hpp,
// bsmr_sparse_attention_qkv_gqa_mfma_16; include/bsmr_hip.h "One-pass grouped-head sparse attention on the MFMA", DESIGN.md
// 25).  The g heads of a KV group walk the same entries of a row of S, so the heads are a dense matrix dimension that costs
// nothing: per tile of entries S^T = Kt_tile Q_group^T and O_group^T = V_tile^T P are small dense products with up to 16
// heads as N.  An opt-in sibling of attnQkvGqa (csrc/attention_qkv_gqa_kernels.hpp) with a contract of its own: the same
// function in another summation order, the weights of the value product rounded to the operands' 16-bit format.
//
// attnQkvGqaMfma: one wave per (BwItem, KV head, sub-group of up to 16 consecutive heads of the group), 4 waves per block
// (4 items, one sub-group); grid y = (b / g) * ceil(g / 16).  A sub-group that ends past the group clamps its surplus head
// indices to the group's last head: those columns compute a duplicate and store nothing.  No LDS.
// Lane l: n = l & 15 is the head of the sub-group it serves, q = l >> 4.  A tile is 32 entries: two score tiles of 16 (the
// halves h = 0, 1), which form one k-step of the value MFMA.
//   scores  S^T = Kt_tile Q^T on v_mfma_f32_16x16x32_f16 / _bf16, K / 32 steps t into one f32x4 from +0 per half.  A operand:
//           elements 32 t + 8 q ... + 7 of Kt[c], c the column of entry 16 h + n of the tile (a lane past the item's end
//           reads row 0).  B operand: the same elements of Q[head n][row], loaded once per item (4 NL VGPRs).  Register i
//           of half h on lane (n, q) is the score of entry 16 h + 4 q + i for head n: z_j, j = 4 h + i.
//   mask    z_j = fl(scale p_j), -inf BY SELECT for an entry past the item's end.
//   softmax per lane for head n, the same bits on the lanes n, n + 16, n + 32, n + 48 - the statements of attnQkvBlocks:
//           tile max = max of the 8 registers in ascending j, then max with lane ^ 16, then lane ^ 32;  m' = max(m, tile
//           max), NaN once any z of the head was NaN;  alpha = expf(fl(m - m')), applied to s and acc only when m' != m
//           and m != -inf;  e_j = expf(fl(z_j - m')), 0 while m' = -inf;  tile sum = (((e_0 + e_1) + e_2) + ... + e_7),
//           then + lane ^ 16, then + lane ^ 32;  s = s + tile sum - the fp32 e, so (m, s) mean what they mean in attnQkv.
//   values  O^T = V^T P on the same instruction.  The k index of the MFMA is a free permutation of the tile's entries:
//           k-slot 8 q + j is the entry of z_j (entry 4 q + j of half 0 for j < 4, entry 4 q + j - 4 of half 1 for j >= 4),
//           so the lane's own 8 weights, narrowed to MODE's format (round to nearest even) and packed in pairs, ARE its B
//           operand: nothing moves.  A operand: per 64-feature chunk the lane loads 8 bytes of V[c_j] at features 64 chunk
//           + 4 n ... + 3 for its 8 k-slots j (the 16 lanes of a q read 128 contiguous bytes of a row) and regroups the 8
//           words pairs with v_perm_b32 into four operands, operand f = feature 4 n + f at the 8 k-slots.  Four MFMAs per
//           chunk and tile, one per f: register i of tile f on lane (n, q) is feature 64 chunk + 16 q + 4 i + f of head n,
//           so a lane owns 16 contiguous features of its head per chunk.  A padding k-slot and a feature past Kv carry
//           zero words BY SELECT: row 0 of V never reaches a row that does not store column 0.
//   skip    the value product of a tile is skipped, wave-uniformly, while no head of the wave has left -inf.
// Non-finite V (a departure from the gather of attnQkvGqa, the rule of a dense softmax @ V): in a tile the wave takes, a
// weight of 0 still enters the MFMA, so a non-finite V[c, k] at a stored entry makes feature k NaN in every head of the
// sub-group that ends the row alive; a head that ends it dead (m = -inf) stores +0.
// Prefetch: the Kt rows of tile t + 1 and the column ids of the next 64 entries fly during tile t's softmax and value
// phase, as in attnQkvGqa.  Every load is branch-free.
// Stores are attnQkvGqa's, per head: a direct item divides (attnDiv), rounds once (bwNarrow) and stores O, m, s; a chunk
// item writes (m_c, s_c, acc_c) to attnQkv's workspace layout [b][slots] indexed by QUERY head, and attnQkvMerge finishes
// split rows unchanged.
// Templates: MODE 0 / 1 = fp16 / bf16; NL = steps the score loop is unrolled for (1, 2, 4, 8: K <= 256; a step past K / 32
// repeats the last piece and its result is dropped by a select); VC = chunks of 64 features (1, 2, 4: Kv <= 256).
// No atomics, one writer per element, every address formed in 64 bits, fp contraction off, the accurate expf; built
// without packed fp32 operations like its siblings (csrc/attention_qkv_gqa_mfma.hip).
#pragma once

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "backward_lists.hpp"   // BwItem, kBwDirect
#include "lowp_device.hpp"      // u32x2, u32x4, f32x4, mfmaLowp, bwNarrow
#include "softmax_device.hpp"   // attnDiv, smExp, smRowMax

namespace bsmr {

constexpr uint32_t kQkvMfmaTile = 32;    // entries per tile: one k-step of the value MFMA
constexpr uint32_t kQkvMfmaHeads = 16;   // heads per wave: the N of both MFMAs

template <int MODE, int NL, int VC>
__global__ void __launch_bounds__(256)
attnQkvGqaMfma(const BwItem* __restrict__ items, uint32_t numItems, const uint32_t* __restrict__ src, float scale,
               const uint16_t* __restrict__ Q, const uint16_t* __restrict__ Kt, const uint16_t* __restrict__ V,
               uint16_t* __restrict__ O, float* __restrict__ mOut, float* __restrict__ sOut, float* __restrict__ partial,
               float* __restrict__ sPart, float* __restrict__ mPart, uint32_t K, uint32_t Kv, uint32_t M, uint32_t N,
               uint32_t numSlots, uint32_t g, uint32_t subs) {
#pragma clang fp contract(off)
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, n = lane & 15u, kq = lane >> 4;
    const uint64_t it = (uint64_t)blockIdx.x * 4u + wave;
    if (it >= numItems) return;   // (whole waves leave: nothing below synchronises across waves)
    const BwItem item = items[it];
    const uint64_t kvHead = blockIdx.y / subs;
    const uint32_t mine = (blockIdx.y % subs) * kQkvMfmaHeads + n;   // this lane's head within its KV group
    const uint64_t head = kvHead * g + min(mine, g - 1u);            // past the group: the last head again, stores nothing
    const uint32_t kc = K / 32u;
    const uint32_t len = item.end - item.begin, nt = (len + kQkvMfmaTile - 1u) / kQkvMfmaTile;
    const uint16_t* kb = Kt + kvHead * N * K + 8u * kq;
    const uint16_t* vb = V + kvHead * N * Kv;

    // this lane's pieces of Q[head][row]: the elements 32 t + 8 kq ... + 7, where it wants them as the B operand
    u32x4 qp[NL] = {};
    if (nt) {   // (an empty row reads nothing: with nnz = 0 the operands may be NULL)
        const uint16_t* qr = Q + (head * M + item.dest) * K + 8u * kq;
#pragma unroll
        for (int i = 0; i < NL; ++i) qp[i] = *reinterpret_cast<const u32x4*>(qr + 32u * min((uint32_t)i, kc - 1u));
    }
    // column ids of the item's entries [64 gr, 64 gr + 64), one per lane: two tiles
    auto groupCols = [&](uint32_t gr) -> uint32_t {
        const uint32_t e = gr * 64u + lane;
        return e < len ? src[item.begin + e] : 0u;
    };
    // the entry of the tile that z_j / k-slot 8 kq + j of this lane stands for
    auto entryOf = [&](int j) -> uint32_t { return (j < 4 ? 0u : 12u) + 4u * kq + (uint32_t)j; };
    // this lane's pieces of the Kt rows of tile t's two halves; cols: the ids of the group tile t lies in.  Branch-free: a
    // lane past the item's end reads row 0, a piece past K / 32 repeats the last one.
    auto loadKt = [&](uint32_t cols, uint32_t t, u32x4 (&kt)[2][NL]) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const uint32_t c = (uint32_t)__shfl((int)cols, (int)((t & 1u) * kQkvMfmaTile + 16u * h + n), 64);
            const uint16_t* row = kb + (uint64_t)c * K;
#pragma unroll
            for (int i = 0; i < NL; ++i) kt[h][i] = *reinterpret_cast<const u32x4*>(row + 32u * min((uint32_t)i, kc - 1u));
        }
    };
    auto score = [&](const u32x4 (&kt)[2][NL], uint32_t t, float (&z)[8]) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            f32x4 p = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int i = 0; i < NL; ++i) {
                const f32x4 next = mfmaLowp<MODE>(kt[h][i], qp[i], p);
                p = (uint32_t)i < kc ? next : p;   // (wave-uniform select: exactly K / 32 steps)
            }
#pragma unroll
            for (int i = 0; i < 4; ++i)
                z[4 * h + i] = t * kQkvMfmaTile + entryOf(4 * h + i) < len ? scale * p[i] : -INFINITY;
        }
    };

    f32x4 acc[VC][4];
#pragma unroll
    for (int c = 0; c < VC; ++c)
#pragma unroll
        for (int f = 0; f < 4; ++f) acc[c][f] = f32x4{0.f, 0.f, 0.f, 0.f};
    float m = -INFINITY, s = 0.0f;
    bool nan = false;

    if (nt) {
        uint32_t cV = groupCols(0), cK = cV, cNext = groupCols(1);
        u32x4 kt[2][NL] = {};
        loadKt(cK, 0, kt);
        float z[8];
        score(kt, 0, z);
        for (uint32_t t = 0; t < nt; ++t) {
            const bool more = t + 1u < nt;
            if (more) {   // tile t + 1's rows of Kt fly during tile t's softmax and value phase
                if (((t + 1u) & 1u) == 0) {
                    cK = cNext;
                    cNext = groupCols((t + 1u) / 2u + 1u);
                }
                loadKt(cK, t + 1u, kt);
            }
            // the online softmax of the tile, head n on this lane
            float tm = z[0];
            bool bad = z[0] != z[0];
#pragma unroll
            for (int j = 1; j < 8; ++j) {
                tm = fmaxf(tm, z[j]);
                bad |= z[j] != z[j];
            }
            tm = fmaxf(tm, __shfl_xor(tm, 16, 64));
            tm = fmaxf(tm, __shfl_xor(tm, 32, 64));
            const uint64_t bads = __ballot(bad);
            nan |= (((bads | (bads >> 16) | (bads >> 32) | (bads >> 48)) >> n) & 1u) != 0;
            const float mNew = smRowMax(fmaxf(m, tm), nan);
            const bool rose = mNew != m;   // (a NaN keeps rescaling: the row stays NaN)
            if (__any(rose)) {
                const float alpha = rose && m != -INFINITY ? expf(m - mNew) : 1.0f;   // (a product with 1 is exact)
                s = s * alpha;
#pragma unroll
                for (int c = 0; c < VC; ++c)
#pragma unroll
                    for (int f = 0; f < 4; ++f) acc[c][f] = acc[c][f] * alpha;
            }
            m = mNew;
            float e[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) e[j] = smExp(z[j], m);
            float ts = e[0];
#pragma unroll
            for (int j = 1; j < 8; ++j) ts = ts + e[j];
            ts = ts + __shfl_xor(ts, 16, 64);
            ts = ts + __shfl_xor(ts, 32, 64);
            s = s + ts;
            // While every head of the wave is at -inf all weights so far are 0: the tile's value product is skipped, and a
            // non-finite row of V behind -inf scores stays out of acc.
            if (__any(m != -INFINITY)) {
                u32x4 w;   // the B operand: k-slot 8 kq + j holds e_j in MODE's format
#pragma unroll
                for (int i = 0; i < 4; ++i) w[i] = bwNarrow<MODE>(e[2 * i], e[2 * i + 1]);
                const uint32_t feat = 4u * n;
                uint32_t col[8];
                bool inside[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const uint32_t at = entryOf(j);
                    col[j] = (uint32_t)__shfl((int)cV, (int)((t & 1u) * kQkvMfmaTile + at), 64);
                    inside[j] = t * kQkvMfmaTile + at < len;
                }
#pragma unroll
                for (int c = 0; c < VC; ++c) {
                    const bool has = 64u * c + feat < Kv;   // (a chunk past Kv, the upper half of a half-full one: +0)
                    const uint32_t off = has ? 64u * c + feat : 0u;
                    u32x2 x[8];
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        const u32x2 got = *reinterpret_cast<const u32x2*>(vb + (uint64_t)col[j] * Kv + off);
                        x[j] = has && inside[j] ? got : u32x2{0u, 0u};
                    }
#pragma unroll
                    for (int f = 0; f < 4; ++f) {   // operand f: feature 4 n + f of the 8 rows, k-slot j in half j of word j / 2
                        const uint32_t sel = f & 1 ? 0x07060302u : 0x05040100u;
                        u32x4 a;
#pragma unroll
                        for (int i = 0; i < 4; ++i) a[i] = __builtin_amdgcn_perm(x[2 * i + 1][f >> 1], x[2 * i][f >> 1], sel);
                        acc[c][f] = mfmaLowp<MODE>(a, w, acc[c][f]);
                    }
                }
            }
            if (more) score(kt, t + 1u, z);
            if (((t + 1u) & 1u) == 0) cV = cK;
        }
    }

    if (mine >= g) return;   // a clamped duplicate: its head is stored by the lanes that own it
    if (item.slot == kBwDirect) {   // the one store of a finished row
        const bool dead = m == -INFINITY;   // an empty row, or every score -inf: s = 0
        const uint64_t row = head * M + item.dest;
        uint16_t* o = O + row * Kv + 16u * kq;
#pragma unroll
        for (int c = 0; c < VC; ++c) {
            if (64u * c + 16u * kq >= Kv) continue;
#pragma unroll
            for (int half = 0; half < 2; ++half) {   // registers 2 half, 2 half + 1 of the four tiles: 8 contiguous features
                u32x4 o16;
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    const int r = 2 * half + i;
                    o16[2 * i] = bwNarrow<MODE>(attnDiv(acc[c][0][r], s, dead), attnDiv(acc[c][1][r], s, dead));
                    o16[2 * i + 1] = bwNarrow<MODE>(attnDiv(acc[c][2][r], s, dead), attnDiv(acc[c][3][r], s, dead));
                }
                *reinterpret_cast<u32x4*>(o + 64u * c + 8u * half) = o16;
            }
        }
        if (kq == 0) {
            mOut[row] = m;
            sOut[row] = s;
        }
    } else {
        const uint64_t slot = head * numSlots + item.slot;
        float* p = partial + slot * Kv + 16u * kq;
#pragma unroll
        for (int c = 0; c < VC; ++c) {
            if (64u * c + 16u * kq >= Kv) continue;
#pragma unroll
            for (int i = 0; i < 4; ++i)   // register i of the four tiles: features 64 c + 16 kq + 4 i ... + 3
                *reinterpret_cast<float4*>(p + 64u * c + 4u * i) =
                    make_float4(acc[c][0][i], acc[c][1][i], acc[c][2][i], acc[c][3][i]);
        }
        if (kq == 0) {
            mPart[slot] = m;
            sPart[slot] = s;
        }
    }
}

}  // namespace bsmr
