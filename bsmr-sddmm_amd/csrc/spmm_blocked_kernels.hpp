// Blocked SpMM over the RPHM's dense 16 x 16 blocks (include/bsmr_hip.h "Blocked SpMM"; csrc/blocked_capi.hpp):
//   Y[r,:] = B[r,:] + R[r,:],  B = the entries of r that lie in its panel's blocks, R = its residue entries.
//
// R is the existing gather (spmmGather / spmmGather16, spmmReduce) over per-row residue lists; for rows of panels with
// blocks it lands in an fp32 staging row of the workspace.  spmmBlocks computes B on v_mfma_f32_16x16x4_f32 and finishes
// the row: one wave owns (panel, group of 64 features) and loops over the panel's blocks with its accumulators in
// registers, so every output element has one writer and nothing is atomic.
//
// Per block, MFMA s (s = 0 .. 3) multiplies the block's columns j = 4s .. 4s + 3:
//   A operand  lane l holds A[i = l & 15][k = l >> 4] = v[cell(i, 4s + k)], or +0 for an empty cell
//   B operand  lane l holds X[col(4s + k)][64 g + 4 n + f],  n = l & 15, for the tile f = 0 .. 3 of the MFMA
// One 16-byte load of X per lane and slice therefore feeds the four tiles, the 16 lanes of a source row read 256
// contiguous bytes, and a block costs 16 MFMAs per 64 features on four independent accumulator chains (the instruction's
// dependent latency is 40 cycles against a 32-cycle issue: two chains would do).  The instruction is a k-ordered fmaf
// chain with one rounding per product, so tile f of lane l ends as the chain over (block, j) in order - the contract.
// At the end lane l holds, for each register i of the four tiles, a float4 of output row 4 (l >> 4) + i at features
// 64 g + 4 n .. + 3: it adds the staged R in fp32 and stores 16 bytes (8 after the one rounding of the 16-bit forms).
//
// Device format (built by bsmr_backward_attach_blocks): per block 64 x uint4 of cells in lane order - cells[b][l][s] =
// block_values[b][l & 15][4 s + (l >> 4)], a CSR index or kBlkNull - and 4 x uint4 of columns, cols[b][k][s] =
// dense_cols[16 b + 4 s + k] (N = padding: nothing is loaded from X, the operand is +0).  A wave reads both with one 16-byte load
// per lane.  The operands of block b + 1 are loaded before the MFMAs of block b, the cells and columns of b + 2 with them.
// All row addresses are formed in 64 bits, the batch is grid y.  No LDS, no inline assembly.
//
// Split panels (bsmr_backward_attach_blocks_split, segment_blocks = S >= 1): a panel's block list is cut into segments of
// S blocks and the work unit of spmmBlocksSeg[16] is (segment, group of 64 features), described by a BlkSegment.  The
// block loop is the same.  A segment that is its whole panel (partial = kBlkNull) finishes as above.  A segment of a split
// panel stores its 16 x 64 fp32 tile into 16 partial rows of the workspace - [b][16 numPartials][K], the segments of a
// panel on consecutive slots - and spmmBlocksFinish[16], one thread per 4 features of a row of a split panel, adds the
// partials in segment order from partial 0, then the staged R, rounds once and stores: still one writer per element of Y
// and of the partial area, nothing atomic.  With S = 0 the handle runs spmmBlocks[16], the panel form, as before.
#pragma once

#include "spmm_kernels.hpp"

namespace bsmr {

constexpr uint32_t kBlkNull = 0xFFFFFFFFu;   // an empty cell; a row of a ragged last panel that does not exist

struct BlkPanel {          // a row panel that has blocks; its ordinal q owns rows [16 q, 16 q + 16) of the staging area
    uint32_t firstBlock;
    uint32_t numBlocks;
};

struct BlkSegment {        // S >= 1: `numBlocks` consecutive blocks of panel ordinal `panel`
    uint32_t firstBlock;
    uint32_t numBlocks;
    uint32_t panel;
    uint32_t partial;      // its slot (16 rows) of the partial area, or kBlkNull: the segment is the whole panel
};

struct BlkSplit {          // a panel cut into numSegments >= 2 segments, on the partial slots firstPartial ...
    uint32_t panel;
    uint32_t firstPartial;
    uint32_t numSegments;
};

// MODE 2: fp32 rows (XT = float); 0 / 1: fp16 / bf16 rows (XT = uint16_t), widened exactly.  Four features of one row.
template <int MODE, typename XT>
__device__ __forceinline__ float4 blkLoadX(const XT* p) {
    if constexpr (MODE == 2) {
        return *reinterpret_cast<const float4*>(p);
    } else {
        const u32x2 w = *reinterpret_cast<const u32x2*>(p);
        float4 x;
        bwWiden<MODE>(w[0], x.x, x.y);
        bwWiden<MODE>(w[1], x.z, x.w);
        return x;
    }
}

struct BlkOperands {
    float a[4];    // A operand of slice s
    float4 x[4];   // B operands of slice s, tiles f = x, y, z, w
};

// Every load is issued unconditionally - eight per lane and block, none waiting for another: an empty cell, a padding
// column and an idle feature column read `zeros` (16 bytes of +0 in the device format) instead of v or X.
template <int MODE, typename XT>
__device__ __forceinline__ void blkFetch(const u32x4 cell, const u32x4 col, const float* __restrict__ vb,
                                         const XT* __restrict__ xs, const float* __restrict__ zeros, bool live, uint32_t N,
                                         uint32_t K, BlkOperands& o) {
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const float* pa = cell[s] != kBlkNull ? vb + cell[s] : zeros;
        const XT* px = live && col[s] < N ? xs + (uint64_t)col[s] * K : reinterpret_cast<const XT*>(zeros);
        o.a[s] = *pa;
        o.x[s] = blkLoadX<MODE, XT>(px);
    }
}

// One wave per (unit, group of 64 features); 4 waves per workgroup, the groups of one unit side by side.  A unit is a
// panel with blocks (SEG false: units = BlkPanel[], its index is the panel's ordinal) or a segment (SEG true: units =
// BlkSegment[]).  R: the staged residue sums [b][16 numPanels][K] fp32; Y in the format of X; P: the partial area (SEG
// only).  panelRows[16 q + i]: the row of S, or kBlkNull past the last non-empty row.
template <int MODE, typename XT, bool SEG>
__device__ __forceinline__ void
blkBody(const void* __restrict__ units, uint32_t numUnits, uint32_t numGroups,
        const uint32_t* __restrict__ panelRows, const u32x4* __restrict__ cells, const u32x4* __restrict__ cols,
        const float* __restrict__ zeros, const float* __restrict__ v, const XT* __restrict__ X,
        const float* __restrict__ R, XT* __restrict__ Y, uint32_t N, uint32_t K, uint64_t vBatch, uint64_t xBatch, uint64_t yBatch, uint64_t rBatch,
        float* __restrict__ P, uint64_t pBatch) {
    const uint32_t lane = threadIdx.x & 63u, n = lane & 15u, kq = lane >> 4;
    const uint64_t unit = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6);
    if (unit >= (uint64_t)numUnits * numGroups) return;   // whole waves leave
    const uint32_t u = (uint32_t)(unit / numGroups), grp = (uint32_t)(unit % numGroups);
    BlkPanel panel;
    uint32_t q = u, part = kBlkNull;
    if constexpr (SEG) {
        const BlkSegment seg = static_cast<const BlkSegment*>(units)[u];
        panel = BlkPanel{seg.firstBlock, seg.numBlocks};
        q = seg.panel;
        part = seg.partial;
    } else {
        panel = static_cast<const BlkPanel*>(units)[u];
    }
    const uint64_t b = blockIdx.y;
    const uint32_t feat = grp * 64u + 4u * n;
    const bool live = feat < K;   // K is a multiple of 32: the last group of K = 32, 96, ... has 8 idle columns
    const XT* xs = X + b * xBatch + feat;
    const float* vb = v + b * vBatch;
    f32x4 acc[4];
#pragma unroll
    for (int f = 0; f < 4; ++f) acc[f] = f32x4{0.f, 0.f, 0.f, 0.f};

    const uint32_t end = panel.firstBlock + panel.numBlocks;
    u32x4 cell = cells[(uint64_t)panel.firstBlock * 64u + lane];
    u32x4 col = cols[(uint64_t)panel.firstBlock * 4u + kq];
    BlkOperands cur;
    blkFetch<MODE, XT>(cell, col, vb, xs, zeros, live, N, K, cur);
    if (panel.firstBlock + 1u < end) {
        cell = cells[(uint64_t)(panel.firstBlock + 1u) * 64u + lane];
        col = cols[(uint64_t)(panel.firstBlock + 1u) * 4u + kq];
    }
    for (uint32_t blk = panel.firstBlock; blk < end; ++blk) {
        BlkOperands next;
        if (blk + 1u < end) {   // wave-uniform
            blkFetch<MODE, XT>(cell, col, vb, xs, zeros, live, N, K, next);
            if (blk + 2u < end) {
                cell = cells[(uint64_t)(blk + 2u) * 64u + lane];
                col = cols[(uint64_t)(blk + 2u) * 4u + kq];
            }
        } else {
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                next.a[s] = 0.f;
                next.x[s] = make_float4(0.f, 0.f, 0.f, 0.f);
            }
        }
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(cur.a[s], cur.x[s].x, acc[0], 0, 0, 0);
            acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(cur.a[s], cur.x[s].y, acc[1], 0, 0, 0);
            acc[2] = __builtin_amdgcn_mfma_f32_16x16x4f32(cur.a[s], cur.x[s].z, acc[2], 0, 0, 0);
            acc[3] = __builtin_amdgcn_mfma_f32_16x16x4f32(cur.a[s], cur.x[s].w, acc[3], 0, 0, 0);
        }
        cur = next;
    }

    if (!live) return;
    if constexpr (SEG) {
        if (part != kBlkNull) {   // wave-uniform: a segment of a split panel leaves its sums to spmmBlocksFinish
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                if (panelRows[16u * q + 4u * kq + (uint32_t)i] == kBlkNull) continue;
                float* dst = P + b * pBatch + ((uint64_t)part * 16u + 4u * kq + (uint32_t)i) * K + feat;
                *reinterpret_cast<float4*>(dst) = make_float4(acc[0][i], acc[1][i], acc[2][i], acc[3][i]);
            }
            return;
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {   // register i of every tile: output row 4 kq + i of the panel
        const uint32_t slot = 16u * q + 4u * kq + (uint32_t)i;
        const uint32_t dest = panelRows[slot];
        if (dest == kBlkNull) continue;
        const float4 r = *reinterpret_cast<const float4*>(R + b * rBatch + (uint64_t)slot * K + feat);
        const float y0 = acc[0][i] + r.x, y1 = acc[1][i] + r.y, y2 = acc[2][i] + r.z, y3 = acc[3][i] + r.w;
        XT* dst = Y + b * yBatch + (uint64_t)dest * K + feat;
        if constexpr (MODE == 2) {
            *reinterpret_cast<float4*>(dst) = make_float4(y0, y1, y2, y3);
        } else {
            u32x2 o;
            o[0] = bwNarrow<MODE>(y0, y1);
            o[1] = bwNarrow<MODE>(y2, y3);
            *reinterpret_cast<u32x2*>(dst) = o;
        }
    }
}

#define BSMR_BLK_PARAMS(XT)                                                                                            \
    const BlkPanel *__restrict__ panels, uint32_t numPanels, uint32_t numGroups, const uint32_t *__restrict__ panelRows,   \
        const u32x4 *__restrict__ cells, const u32x4 *__restrict__ cols, const float *__restrict__ zeros,                  \
        const float *__restrict__ v, const XT *__restrict__ X, const float *__restrict__ R, XT *__restrict__ Y,            \
        uint32_t N, uint32_t K, uint64_t vBatch, uint64_t xBatch, uint64_t yBatch, uint64_t rBatch
#define BSMR_BLK_ARGS \
    panels, numPanels, numGroups, panelRows, cells, cols, zeros, v, X, R, Y, N, K, vBatch, xBatch, yBatch, rBatch

__global__ void __launch_bounds__(256) spmmBlocks(BSMR_BLK_PARAMS(float)) {
    blkBody<2, float, false>(BSMR_BLK_ARGS, nullptr, 0);
}

template <int MODE>
__global__ void __launch_bounds__(256) spmmBlocks16(BSMR_BLK_PARAMS(uint16_t)) {
    blkBody<MODE, uint16_t, false>(BSMR_BLK_ARGS, nullptr, 0);
}

#undef BSMR_BLK_PARAMS
#undef BSMR_BLK_ARGS

// The segment form: segs[numSegs] in panel order, the segments of a panel in block order.
#define BSMR_SEG_PARAMS(XT)                                                                                            \
    const BlkSegment *__restrict__ segs, uint32_t numSegs, uint32_t numGroups, const uint32_t *__restrict__ panelRows,     \
        const u32x4 *__restrict__ cells, const u32x4 *__restrict__ cols, const float *__restrict__ zeros,                  \
        const float *__restrict__ v, const XT *__restrict__ X, const float *__restrict__ R, XT *__restrict__ Y,            \
        uint32_t N, uint32_t K, uint64_t vBatch, uint64_t xBatch, uint64_t yBatch, uint64_t rBatch,                        \
        float *__restrict__ P, uint64_t pBatch
#define BSMR_SEG_ARGS \
    segs, numSegs, numGroups, panelRows, cells, cols, zeros, v, X, R, Y, N, K, vBatch, xBatch, yBatch, rBatch, P, pBatch

__global__ void __launch_bounds__(256) spmmBlocksSeg(BSMR_SEG_PARAMS(float)) { blkBody<2, float, true>(BSMR_SEG_ARGS); }

template <int MODE>
__global__ void __launch_bounds__(256) spmmBlocksSeg16(BSMR_SEG_PARAMS(uint16_t)) {
    blkBody<MODE, uint16_t, true>(BSMR_SEG_ARGS);
}

#undef BSMR_SEG_PARAMS
#undef BSMR_SEG_ARGS

// One thread per 4 features of one row of a split panel: B = ((p0 + p1) + p2) + ... in segment order, Y = fl(B + R),
// rounded once in the 16-bit forms.  The rows of a ragged panel that do not exist have no partials and are skipped.
template <int MODE, typename XT>
__device__ __forceinline__ void
blkFinishBody(const BlkSplit* __restrict__ splits, uint32_t numSplits, const uint32_t* __restrict__ panelRows,
              const float* __restrict__ P, const float* __restrict__ R, XT* __restrict__ Y, uint32_t K, uint64_t pBatch,
              uint64_t rBatch, uint64_t yBatch) {
    const uint32_t quads = K / 4u;
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (uint64_t)numSplits * 16u * quads) return;
    const uint32_t feat = 4u * (uint32_t)(t % quads);
    const uint64_t row = t / quads;
    const BlkSplit sp = splits[row / 16u];
    const uint32_t i = (uint32_t)(row % 16u);
    const uint32_t slot = 16u * sp.panel + i;
    const uint32_t dest = panelRows[slot];
    if (dest == kBlkNull) return;
    const uint64_t b = blockIdx.y;
    const float* p = P + b * pBatch + ((uint64_t)sp.firstPartial * 16u + i) * K + feat;
    float4 acc = *reinterpret_cast<const float4*>(p);
    for (uint32_t k = 1; k < sp.numSegments; ++k) {
        p += 16ull * K;
        const float4 c = *reinterpret_cast<const float4*>(p);
        acc.x += c.x;
        acc.y += c.y;
        acc.z += c.z;
        acc.w += c.w;
    }
    const float4 r = *reinterpret_cast<const float4*>(R + b * rBatch + (uint64_t)slot * K + feat);
    const float y0 = acc.x + r.x, y1 = acc.y + r.y, y2 = acc.z + r.z, y3 = acc.w + r.w;
    XT* dst = Y + b * yBatch + (uint64_t)dest * K + feat;
    if constexpr (MODE == 2) {
        *reinterpret_cast<float4*>(dst) = make_float4(y0, y1, y2, y3);
    } else {
        u32x2 o;
        o[0] = bwNarrow<MODE>(y0, y1);
        o[1] = bwNarrow<MODE>(y2, y3);
        *reinterpret_cast<u32x2*>(dst) = o;
    }
}

#define BSMR_FIN_PARAMS(XT)                                                                                            \
    const BlkSplit *__restrict__ splits, uint32_t numSplits, const uint32_t *__restrict__ panelRows,                       \
        const float *__restrict__ P, const float *__restrict__ R, XT *__restrict__ Y, uint32_t K, uint64_t pBatch,         \
        uint64_t rBatch, uint64_t yBatch
#define BSMR_FIN_ARGS splits, numSplits, panelRows, P, R, Y, K, pBatch, rBatch, yBatch

__global__ void __launch_bounds__(256) spmmBlocksFinish(BSMR_FIN_PARAMS(float)) { blkFinishBody<2, float>(BSMR_FIN_ARGS); }

template <int MODE>
__global__ void __launch_bounds__(256) spmmBlocksFinish16(BSMR_FIN_PARAMS(uint16_t)) {
    blkFinishBody<MODE, uint16_t>(BSMR_FIN_ARGS);
}

#undef BSMR_FIN_PARAMS
#undef BSMR_FIN_ARGS

}  // namespace bsmr
