// One-pass sparse attention over the RPHM's dense 16 x 16 blocks (csrc/attention_qkv_blocked_capi.hpp,
// bsmr_sparse_attention_qkv_blocked_16; include/bsmr_hip.h "One-pass sparse attention over blocks").
//
// The entries of a row of S that lie in its panel's blocks are served here, both products on the MFMA; its residue entries
// go through attnQkv (csrc/attention_qkv_kernels.hpp) unchanged, every chunk to a partial slot.  attnQkvBlkMerge merges
// the partials of a row.  No score is written.
//
// attnQkvBlocks: one wave per (unit, slab of 64 G features of Kv), 4 waves per workgroup, batches in grid y.  A unit is a
// panel with blocks (BlkPanel) or, on a handle attached with segment_blocks >= 1, a BlkSegment.  The wave loops over the
// unit's blocks with (m, s, acc) of the panel's 16 rows in registers and stores them as a partial at the end, always.
// Lane l: n = l & 15 is the panel row it serves, q = l >> 4.  Both MFMAs are the transposed products:
//   scores  S^T = Kt_blk Q_panel^T on v_mfma_f32_16x16x32_f16 / _bf16, K / 32 steps t into one f32x4 from +0.  A operand:
//           elements 32 t + 8 q ... + 7 of the row Kt[c], c = the block's column 4 (n & 3) + (n >> 2) - the word 16 blk + n
//           of `cols`, one 16-byte load per step, the 4 lanes of a column read 64 contiguous bytes.  B operand: the same
//           elements of Q[panel row n] (registers up to K = 128, else the wave's slice of LDS; a row that does not exist
//           is +0).  Register i of lane l is then the score p of panel row n at block column 4 i + q: the cell
//           cells[blk][l][i], its column cols[blk][q][i] - the attached format as it is.
//   mask    z_i = fl(scale p_i) for a stored cell, -inf BY SELECT for an empty cell (a padding column has only empty
//           cells; its Kt load reads row 0): a NaN row of Kt reaches only the rows that store that column.
//   softmax per lane for row n, the same bits on the lanes n, n + 16, n + 32, n + 48:
//           tile max = max of the 4 registers, then max with lane ^ 16, then lane ^ 32;  m' = max(m, tile max), NaN once
//           any z of the row was NaN (the flag rule of the sparse row softmax);  alpha = expf(fl(m - m')), 1 while m =
//           -inf or m' = m;  s = fl(s alpha), acc = fl(acc alpha) (the code is skipped when no row of the wave rose: a
//           product with 1 is exact);  e_i = expf(fl(z_i - m')), 0 while m' = -inf;
//           tile sum = ((e_0 + e_1) + e_2) + e_3, then + lane ^ 16, then + lane ^ 32;  s = s + tile sum.
//   values  O^T = V_blk^T P^T on v_mfma_f32_16x16x4_f32: for slice i = 0 .. 3 the B operand is the lane's own e_i
//           (B[k = q][n], the weight of row n at column 4 i + q: nothing moves), the A operand comes from one 8-byte load
//           per lane, slice and 64-feature group g: V[cols[blk][q][i]] at features 64 g + 4 n ... + 3, widened exactly,
//           component f to tile f (the 16 lanes of a source row read 128 contiguous bytes; a padding column and a
//           feature past Kv give +0).  Register i of tile f of lane l is output row n, feature 64 g + 16 q + 4 i + f.
//           Per feature: the MFMA's k-ordered fmaf chain over (block, slice, k = q) from +0, one rounding per step,
//           interleaved with the rescales above.
// Empty-cell rule (that of the blocked SpMM): e = 0 still enters the value MFMA, so a non-finite V[c, k] makes acc_k NaN
// in every row of a unit that holds c as a block column, stored or not.  A row whose m is still -inf at the unit's end
// stores m = -inf and the merge skips that partial, so the NaN reaches O only for rows that store a cell in that unit.
// Prefetch: the cells and columns of block b + 2 and the Kt rows of block b + 1 fly during block b's softmax and value
// MFMAs; the V rows of block b are requested in front of them.  Every load is unconditional.
// Templates: MODE 0 / 1 = fp16 / bf16; NL = steps the score loop is unrolled for (1, 2, 4, 8, 16; K / 32 <= NL, a step
// past K / 32 repeats the last piece and its result is dropped by a select); G = 64-feature groups per wave (1, 2).
// Slabs recompute the scores: every slab of a unit holds the same (m, s), slab 0 stores them.
//
// attnQkvBlkMerge: one thread per 4 features of a row of a panel with blocks (BsmrAttnBlkRow).  The row's partials in
// the order residue chunks (chunk order), then block units (segment order); the statements of attnQkvMerge: m = max (NaN
// if any is), beta = expf(fl(m_c - m)), a partial with m_c = -inf is skipped, s and acc summed from +0, one IEEE division,
// one bwNarrow, m and s stored by the thread of feature 0.
// No atomics, one writer per element, every address formed in 64 bits, fp contraction off, the accurate expf.
#pragma once

#include "attention_qkv_kernels.hpp"
#include "attention_qkv_launch.hpp"   // BsmrAttnBlkRow
#include "blocked_format.hpp"         // BlkPanel, BlkSegment, kBlkNull

namespace bsmr {

template <int MODE, int NL, int G>
__global__ void __launch_bounds__(256)
attnQkvBlocks(const void* __restrict__ units, uint32_t numUnits, uint32_t segments, uint32_t numSlabs,
              const uint32_t* __restrict__ panelRows, const u32x4* __restrict__ cells, const u32x4* __restrict__ cols,
              const float* __restrict__ zeros, float scale, const uint16_t* __restrict__ Q, const uint16_t* __restrict__ Kt,
              const uint16_t* __restrict__ V, float* __restrict__ bPart, float* __restrict__ bs, float* __restrict__ bm,
              uint32_t K, uint32_t Kv, uint32_t M, uint32_t N) {
#pragma clang fp contract(off)
    constexpr bool QLDS = NL > 4;
    // a staged row of Q: 4 NL pieces of 16 bytes; piece j of row n lies at j ^ n, so that the 16 rows of one ds_read_b128
    // spread over all banks (a lane reads back only what it stored itself: any bijection serves)
    constexpr uint32_t kRowPieces = 4u * NL;
    __shared__ u32x4 qLds[QLDS ? 4u * 16u * kRowPieces : 1u];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, n = lane & 15u, kq = lane >> 4;
    const uint64_t work = (uint64_t)blockIdx.x * 4u + wave;
    if (work >= (uint64_t)numUnits * numSlabs) return;   // (whole waves leave: nothing below synchronises across waves)
    const uint32_t u = (uint32_t)(work / numSlabs), slab = (uint32_t)(work % numSlabs);
    uint32_t first, count, panel = u;
    if (segments) {   // kernel-uniform
        const BlkSegment sg = static_cast<const BlkSegment*>(units)[u];
        first = sg.firstBlock;
        count = sg.numBlocks;
        panel = sg.panel;
    } else {
        const BlkPanel pn = static_cast<const BlkPanel*>(units)[u];
        first = pn.firstBlock;
        count = pn.numBlocks;
    }
    const uint64_t b = blockIdx.y;
    const uint32_t kc = K / 32u;
    const uint32_t row = panelRows[16u * panel + n];
    const bool exists = row != kBlkNull;   // a ragged panel's missing row: Q = +0, every cell empty, nothing stored

    // this lane's pieces of Q[row]: the elements 32 t + 8 kq ... + 7, where it will want them as the B operand
    const uint16_t* qr = exists ? Q + (b * M + row) * K + 8u * kq : reinterpret_cast<const uint16_t*>(zeros);
    u32x4 q[QLDS ? 1 : NL] = {};
    u32x4* qMine = qLds + (wave * 16u + n) * kRowPieces;
#pragma unroll
    for (int i = 0; i < NL; ++i) {
        const u32x4 piece = *reinterpret_cast<const u32x4*>(qr + (exists ? 32u * min((uint32_t)i, kc - 1u) : 0u));
        if constexpr (QLDS) qMine[(4u * i + kq) ^ n] = piece;
        else q[i] = piece;
    }
    const uint16_t* kb = Kt + b * N * K + 8u * kq;
    auto loadKt = [&](uint32_t c, u32x4 (&kt)[NL]) {
        const uint16_t* kr = kb + (uint64_t)(c < N ? c : 0u) * K;   // (a padding column reads row 0; all its cells are empty)
#pragma unroll
        for (int i = 0; i < NL; ++i) kt[i] = *reinterpret_cast<const u32x4*>(kr + 32u * min((uint32_t)i, kc - 1u));
    };
    auto score = [&](const u32x4 (&kt)[NL], const u32x4 cell, float (&z)[4]) {
        f32x4 p = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int i = 0; i < NL; ++i) {
            u32x4 qi;
            if constexpr (QLDS) qi = qMine[(4u * i + kq) ^ n];
            else qi = q[i];
            const f32x4 next = mfmaLowp<MODE>(kt[i], qi, p);
            p = (uint32_t)i < kc ? next : p;   // (wave-uniform select: exactly K / 32 steps)
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) z[i] = cell[i] != kBlkNull ? scale * p[i] : -INFINITY;
    };
    // the rows of V of one block: slice i, group g
    const uint32_t feat0 = slab * (64u * G) + 4u * n;
    const uint16_t* vb = V + b * N * Kv + feat0;
    auto loadV = [&](const u32x4 col, u32x2 (&x)[4][G]) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int g = 0; g < G; ++g) {
                const bool live = col[i] < N && feat0 + 64u * g < Kv;
                const uint16_t* p = live ? vb + (uint64_t)col[i] * Kv + 64u * g : reinterpret_cast<const uint16_t*>(zeros);
                x[i][g] = *reinterpret_cast<const u32x2*>(p);
            }
    };

    f32x4 acc[G][4];
#pragma unroll
    for (int g = 0; g < G; ++g)
#pragma unroll
        for (int f = 0; f < 4; ++f) acc[g][f] = f32x4{0.f, 0.f, 0.f, 0.f};
    float m = -INFINITY, s = 0.0f;
    bool nan = false;

    const uint32_t* colWords = reinterpret_cast<const uint32_t*>(cols);
    const uint32_t end = first + count;
    u32x4 col = cols[(uint64_t)first * 4u + kq];
    u32x4 cellN = cells[(uint64_t)first * 64u + lane], colN = col;
    uint32_t ckN = colWords[(uint64_t)first * 16u + n];
    u32x4 kt[NL] = {};
    loadKt(ckN, kt);
    float z[4];
    {
        const u32x4 cell = cellN;
        if (first + 1u < end) {
            cellN = cells[(uint64_t)(first + 1u) * 64u + lane];
            colN = cols[(uint64_t)(first + 1u) * 4u + kq];
            ckN = colWords[(uint64_t)(first + 1u) * 16u + n];
        }
        score(kt, cell, z);
    }
    for (uint32_t blk = first; blk < end; ++blk) {
        const bool more = blk + 1u < end;   // wave-uniform
        u32x2 x[4][G];
        loadV(col, x);
        if (more) loadKt(ckN, kt);
        u32x4 cell2 = cellN, col2 = colN;
        uint32_t ck2 = ckN;
        if (blk + 2u < end) {
            cell2 = cells[(uint64_t)(blk + 2u) * 64u + lane];
            col2 = cols[(uint64_t)(blk + 2u) * 4u + kq];
            ck2 = colWords[(uint64_t)(blk + 2u) * 16u + n];
        }
        // the online softmax of the block's 16 x 16 tile, row n on this lane
        float tm = fmaxf(fmaxf(fmaxf(z[0], z[1]), z[2]), z[3]);
        tm = fmaxf(tm, __shfl_xor(tm, 16, 64));
        tm = fmaxf(tm, __shfl_xor(tm, 32, 64));
        const uint64_t bad = __ballot(z[0] != z[0] || z[1] != z[1] || z[2] != z[2] || z[3] != z[3]);
        nan |= (((bad | (bad >> 16) | (bad >> 32) | (bad >> 48)) >> n) & 1u) != 0;
        const float mNew = smRowMax(fmaxf(m, tm), nan);
        const bool rose = mNew != m;   // (a NaN keeps rescaling: the row stays NaN)
        if (__any(rose)) {
            const float alpha = rose && m != -INFINITY ? expf(m - mNew) : 1.0f;
            s = s * alpha;
#pragma unroll
            for (int g = 0; g < G; ++g)
#pragma unroll
                for (int f = 0; f < 4; ++f) acc[g][f] = acc[g][f] * alpha;
        }
        m = mNew;
        float e[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) e[i] = smExp(z[i], m);
        float ts = ((e[0] + e[1]) + e[2]) + e[3];
        ts = ts + __shfl_xor(ts, 16, 64);
        ts = ts + __shfl_xor(ts, 32, 64);
        s = s + ts;
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int g = 0; g < G; ++g) {
                float a0, a1, a2, a3;
                bwWiden<MODE>(x[i][g][0], a0, a1);
                bwWiden<MODE>(x[i][g][1], a2, a3);
                acc[g][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, e[i], acc[g][0], 0, 0, 0);
                acc[g][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, e[i], acc[g][1], 0, 0, 0);
                acc[g][2] = __builtin_amdgcn_mfma_f32_16x16x4f32(a2, e[i], acc[g][2], 0, 0, 0);
                acc[g][3] = __builtin_amdgcn_mfma_f32_16x16x4f32(a3, e[i], acc[g][3], 0, 0, 0);
            }
        if (more) score(kt, cellN, z);
        col = colN;
        cellN = cell2;
        colN = col2;
        ckN = ck2;
    }

    if (!exists) return;
    const uint64_t slot = (b * numUnits + u) * 16u + n;
    float* dst = bPart + slot * Kv + slab * (64u * G) + 16u * kq;
#pragma unroll
    for (int g = 0; g < G; ++g)
#pragma unroll
        for (int i = 0; i < 4; ++i)   // register i of the four tiles: features 64 g + 16 kq + 4 i ... + 3 of row n
            if (slab * (64u * G) + 64u * g + 16u * kq + 4u * i < Kv)
                *reinterpret_cast<float4*>(dst + 64u * g + 4u * i) =
                    make_float4(acc[g][0][i], acc[g][1][i], acc[g][2][i], acc[g][3][i]);
    if (slab == 0 && kq == 0) {
        bm[slot] = m;
        bs[slot] = s;
    }
}

template <int MODE>
__global__ void __launch_bounds__(256)
attnQkvBlkMerge(const BsmrAttnBlkRow* __restrict__ rows, uint32_t numRows, const float* __restrict__ partial,
                const float* __restrict__ sPart, const float* __restrict__ mPart, uint32_t numSlots,
                const float* __restrict__ bPart, const float* __restrict__ bs, const float* __restrict__ bm,
                uint32_t numUnits, uint16_t* __restrict__ O, float* __restrict__ mOut, float* __restrict__ sOut, uint32_t Kv,
                uint32_t M) {
#pragma clang fp contract(off)
    const uint32_t q = Kv / 4u;
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= (uint64_t)numRows * q) return;
    const BsmrAttnBlkRow r = rows[i / q];
    const uint64_t c = (i % q) * 4u;
    const uint64_t b = blockIdx.y, res0 = b * numSlots + r.resFirst, blk0 = b * numUnits * 16u + r.blkFirst;
    const uint32_t total = r.resCount + r.blkCount;
    // partial k of the row: its residue chunks first, then its block units, 16 rows apart
    auto mAt = [&](uint32_t k) { return k < r.resCount ? mPart[res0 + k] : bm[blk0 + 16ull * (k - r.resCount)]; };
    auto sAt = [&](uint32_t k) { return k < r.resCount ? sPart[res0 + k] : bs[blk0 + 16ull * (k - r.resCount)]; };
    auto accAt = [&](uint32_t k) {
        const float* p = k < r.resCount ? partial + (res0 + k) * Kv : bPart + (blk0 + 16ull * (k - r.resCount)) * Kv;
        return *reinterpret_cast<const float4*>(p + c);
    };
    float m = -INFINITY;
    bool nan = false;
    for (uint32_t k = 0; k < total; ++k) {
        const float mk = mAt(k);
        m = fmaxf(m, mk);
        nan |= mk != mk;
    }
    m = smRowMax(m, nan);
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    float s = 0.0f;
    for (uint32_t k = 0; k < total; ++k) {
        const float mk = mAt(k);
        if (mk == -INFINITY) continue;   // beta = 0: skipped, not multiplied (the empty-cell rule stops here)
        const float beta = expf(mk - m);
        const float4 x = accAt(k);
        s = s + sAt(k) * beta;
        acc.x = acc.x + x.x * beta;
        acc.y = acc.y + x.y * beta;
        acc.z = acc.z + x.z * beta;
        acc.w = acc.w + x.w * beta;
    }
    const uint64_t row = b * M + r.dest;
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
