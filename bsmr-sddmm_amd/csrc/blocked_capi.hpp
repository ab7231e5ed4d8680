// Blocked SpMM (include/bsmr_hip.h "Blocked SpMM"): the check of an RPHM against a CSR, the device format that
// bsmr_backward_attach_blocks builds from it, and the two calls that run csrc/spmm_blocked_kernels.hpp.
//
// Host side, no device call before everything is validated:
//   * blockedCheck walks every block cell and every residue entry once, marks the CSR index it names and compares its
//     (row, column) with the CSR - so that the kernel can trust every index it is given;
//   * the residue lists are not taken from the RPHM's sparse_* arrays (whose relative rows are not sorted within a
//     panel): the CSR indices that no block cell holds, in ascending order, ARE the residue row by row in ascending CSR
//     index.  Every row of S gets a list (an empty one zeroes its destination), cut into chunks of BSMR_BACKWARD_CHUNK
//     exactly as buildItems cuts the rows; rows are scheduled in reordered_rows order, then the empty rows;
//   * cells and columns are transposed into the lane order of the kernel.
//   * segment_blocks = S >= 1: every panel's block list is cut into ceil(nb / S) segments; a panel of one segment keeps
//     the finish of the panel form, the segments of a split panel get consecutive slots of the partial area.
// Workspace of a call (K, b), in floats: [b][numSlots][K] chunk partials of the residue, then [b][16 numPanels][K]
// staging rows, then [b][16 numPartials][K] segment partials (workFloatsFor covers all three on a handle with attached
// blocks).
// Included at the end of bsmr_capi.hip, after backward_capi.hpp.
#pragma once

namespace {

struct BlockedHost {
    bsmr_blocked_stats stats{};
    std::vector<uint8_t> inBlock;     // [nnz] 1: the entry lies in a block cell
    std::vector<uint32_t> resOffsets; // [M + 1] residue entries before each row
};

// segments of a panel of nb >= 1 blocks
uint64_t segmentsOf(uint32_t nb, uint32_t S) { return S ? ((uint64_t)nb + S - 1u) / S : 1u; }

int blockedCheck(uint32_t M, uint32_t N, uint32_t nnz, const uint32_t* ro, const uint32_t* ci, const bsmr_rphm_desc* d,
                 uint32_t S, BlockedHost& h) {
    if (!d) return BSMR_ERR_INVALID_ARG;
    if (int st = checkCsr(M, N, nnz, ro, ci)) return st;
    if (d->M != M || d->N != N || d->nnz != nnz) return BSMR_ERR_INVALID_ARG;
    const uint32_t P = d->num_row_panels, rowsIn = d->num_nonzero_rows;
    if (!d->block_offsets || !d->sparse_value_offsets || (rowsIn && !d->reordered_rows)) return BSMR_ERR_INVALID_ARG;
    if (rowsIn > M || P != (uint32_t)(((uint64_t)rowsIn + 15u) / 16u)) return BSMR_ERR_BAD_PLAN;
    const uint32_t *bo = d->block_offsets, *so = d->sparse_value_offsets;
    if (bo[0] != 0 || so[0] != 0) return BSMR_ERR_BAD_PLAN;
    for (uint32_t p = 0; p < P; ++p)
        if (bo[p + 1] < bo[p] || so[p + 1] < so[p]) return BSMR_ERR_BAD_PLAN;
    const uint64_t blocks = bo[P], residue = so[P];
    if (blocks && (!d->dense_cols || !d->block_values)) return BSMR_ERR_INVALID_ARG;
    if (residue && (!d->sparse_values || !d->sparse_relative_rows || !d->sparse_col_indices)) return BSMR_ERR_INVALID_ARG;
    if (residue > nnz) return BSMR_ERR_BAD_PLAN;
    {
        std::vector<uint8_t> seenRow(M, 0);
        for (uint32_t i = 0; i < rowsIn; ++i) {
            const uint32_t r = d->reordered_rows[i];
            if (r >= M || seenRow[r]) return BSMR_ERR_BAD_PLAN;
            seenRow[r] = 1;
        }
    }
    bsmr_blocked_stats& s = h.stats;
    s = bsmr_blocked_stats{};
    s.panels = P;
    s.blocks = blocks;
    s.residue_entries = residue;
    s.segment_blocks = S;
    uint64_t segments = 0;
    h.inBlock.assign(nnz, 0);
    std::vector<uint8_t> seen(nnz, 0);
    // entry t must be stored at (row, col) of the CSR, once
    auto claim = [&](uint32_t t, uint32_t slot, uint32_t col) {
        if (t >= nnz || slot >= rowsIn || seen[t]) return false;
        const uint32_t r = d->reordered_rows[slot];
        if (t < ro[r] || t >= ro[r + 1] || ci[t] != col) return false;
        seen[t] = 1;
        return true;
    };
    uint64_t claimed = 0;
    for (uint32_t p = 0; p < P; ++p) {
        const uint32_t nb = bo[p + 1] - bo[p];
        s.panels_with_blocks += nb ? 1u : 0u;
        s.max_blocks_per_panel = std::max(s.max_blocks_per_panel, nb);
        s.split_panels += S && nb > S ? 1u : 0u;
        segments += nb ? segmentsOf(nb, S) : 0u;
        for (uint64_t b = bo[p]; b < bo[p + 1]; ++b) {
            const uint32_t* cols = d->dense_cols + 16u * b;
            for (uint32_t j = 0; j < 16; ++j) {
                if (cols[j] > N) return BSMR_ERR_BAD_PLAN;
                s.padding_columns += cols[j] == N ? 1u : 0u;
            }
            const uint32_t* cell = d->block_values + 256u * b;
            for (uint32_t i = 0; i < 16; ++i)
                for (uint32_t j = 0; j < 16; ++j) {
                    const uint32_t t = cell[16u * i + j];
                    if (t == bsmr::kBlkNull) continue;
                    if (cols[j] == N || !claim(t, 16u * p + i, cols[j])) return BSMR_ERR_BAD_PLAN;
                    h.inBlock[t] = 1;
                    ++s.block_entries;
                }
        }
        for (uint64_t e = so[p]; e < so[p + 1]; ++e) {
            const uint32_t rel = d->sparse_relative_rows[e];
            if (rel >= 16u || !claim(d->sparse_values[e], 16u * p + rel, d->sparse_col_indices[e])) return BSMR_ERR_BAD_PLAN;
        }
        claimed = s.block_entries + so[p + 1];
    }
    if (claimed != nnz) return BSMR_ERR_BAD_PLAN;   // every claim was a different entry: equal counts = a partition
    s.segments = (uint32_t)segments;                // at most one per block: blocks < 2^32
    s.max_blocks_per_segment = S ? std::min(S, s.max_blocks_per_panel) : s.max_blocks_per_panel;
    constexpr uint32_t C = BSMR_BACKWARD_CHUNK;
    h.resOffsets.assign((size_t)M + 1u, 0u);
    for (uint32_t r = 0; r < M; ++r) {
        uint32_t len = 0;
        for (uint32_t t = ro[r]; t < ro[r + 1]; ++t) len += h.inBlock[t] ? 0u : 1u;
        h.resOffsets[r + 1] = h.resOffsets[r] + len;
        s.max_residue_row = std::max(s.max_residue_row, len);
        s.split_residue_rows += len > C ? 1u : 0u;
        s.residue_items += std::max(1u, (len + C - 1u) / C);
    }
    return BSMR_OK;
}

// modeOk: what the entry point accepts as compute mode, tested where bsmr_spmm_16 tests it (checkSpmmCall)
int checkBlockedCall(const bsmr_backward* bw, uint32_t K, bool modeOk, uint32_t nb, const void* v, const void* X, const void* Y) {
    if (int st = checkBackwardCall(bw, K, nb)) return st;
    if (!modeOk) return BSMR_ERR_INVALID_ARG;
    if (!bw->blocked) return BSMR_ERR_BAD_PLAN;
    const bool reads = bw->nnz != 0;   // as bsmr_spmm: nnz = 0 reads neither v nor X, Y is still zeroed
    if ((reads && (!v || !X)) || !Y || !aligned4(v) || !aligned16(X) || !aligned16(Y)) return BSMR_ERR_INVALID_ARG;
    return BSMR_OK;
}

// mode: BSMR_COMPUTE_F32 for fp32 X / Y, else the 16-bit format of both.  The workspace is already large enough.
int runBlocked(bsmr_backward* bw, uint32_t K, const float* v, const void* X, void* Y, uint32_t nb, int mode, hipStream_t s) {
    const BwBlocked& f = *bw->blocked;
    const bool y16 = mode != BSMR_COMPUTE_F32;
    const uint16_t* X16 = static_cast<const uint16_t*>(X);
    uint16_t* Y16 = static_cast<uint16_t*>(Y);
    const uint64_t nnz = bw->nnz;
    const uint64_t xB = (uint64_t)bw->N * K, yB = (uint64_t)bw->M * K, pB = (uint64_t)f.numSlots * K;
    const uint64_t rB = 16ull * f.numPanels * K, sB = 16ull * f.numPartials * K;
    float* partial = bw->work;
    float* stage = bw->work + pB * nb;
    float* segPartial = stage + rB * nb;
    // R of the rows outside panels with blocks is their row of Y; R of the others waits in fp32 for the block chain
    const GatherLists toY{f.items[0], f.numItems[0], f.splits[0], f.numSplits[0], f.resCols, f.resIdx};
    const GatherLists toStage{f.items[1], f.numItems[1], f.splits[1], f.numSplits[1], f.resCols, f.resIdx};
    if (int st = runGather(bw, toY, K, v, X, Y, partial, nnz, xB, yB, pB, nb, s, {mode, y16})) return st;
    if (int st = runGather(bw, toStage, K, v, X, stage, partial, nnz, xB, rB, pB, nb, s, {mode, false})) return st;
    if (!f.numPanels) return BSMR_OK;
    const uint32_t groups = (K + 63u) / 64u;
    if (!f.segmentBlocks) {   // the panel form
        const uint64_t units = (uint64_t)f.numPanels * groups;
        const dim3 grid((uint32_t)((units + 3u) / 4u), nb);
        auto launch = [&](auto kernel, auto* x, auto* y) {
            hipLaunchKernelGGL(kernel, grid, dim3(256), 0, s, f.panels, f.numPanels, groups, f.panelRows, f.cells, f.cols,
                               f.zeros, v, x, stage, y, bw->N, K, nnz, xB, yB, rB);
        };
        if (!y16) launch(bsmr::spmmBlocks, static_cast<const float*>(X), static_cast<float*>(Y));
        else withMode(mode, [&](auto MODE) { launch(bsmr::spmmBlocks16<MODE()>, X16, Y16); });
        BSMR_HIP(hipGetLastError());
        return BSMR_OK;
    }
    // the segment form; the finishing kernel only where a panel is split
    const uint64_t units = (uint64_t)f.numSegs * groups;
    const uint64_t finThreads = 16ull * f.numSplitPanels * (K / 4u);
    const dim3 grid((uint32_t)((units + 3u) / 4u), nb), finGrid((uint32_t)((finThreads + 255u) / 256u), nb);
    auto launch = [&](auto kernel, auto finish, auto* x, auto* y) {
        hipLaunchKernelGGL(kernel, grid, dim3(256), 0, s, f.segs, f.numSegs, groups, f.panelRows, f.cells, f.cols, f.zeros, v,
                           x, stage, y, bw->N, K, nnz, xB, yB, rB, segPartial, sB);
        if (f.numSplitPanels)
            hipLaunchKernelGGL(finish, finGrid, dim3(256), 0, s, f.splitPanels, f.numSplitPanels, f.panelRows, segPartial,
                               stage, y, K, sB, rB, yB);
    };
    if (!y16) launch(bsmr::spmmBlocksSeg, bsmr::spmmBlocksFinish, static_cast<const float*>(X), static_cast<float*>(Y));
    else withMode(mode, [&](auto MODE) { launch(bsmr::spmmBlocksSeg16<MODE()>, bsmr::spmmBlocksFinish16<MODE()>, X16, Y16); });
    BSMR_HIP(hipGetLastError());
    return BSMR_OK;
}

}  // namespace

extern "C" {

int bsmr_blocked_check_split(uint32_t M, uint32_t N, uint32_t nnz, const uint32_t* row_offsets, const uint32_t* col_indices,
                             const bsmr_rphm_desc* desc, uint32_t segment_blocks, bsmr_blocked_stats* out, size_t out_size) {
    if (!out) return BSMR_ERR_INVALID_ARG;
    try {
        BlockedHost h;
        if (int st = blockedCheck(M, N, nnz, row_offsets, col_indices, desc, segment_blocks, h)) return st;
        memcpy(out, &h.stats, std::min(out_size, sizeof(h.stats)));   // (the struct only grows at its end)
    } catch (const std::bad_alloc&) {
        return BSMR_ERR_OOM;
    }
    return BSMR_OK;
}

int bsmr_blocked_check(uint32_t M, uint32_t N, uint32_t nnz, const uint32_t* row_offsets, const uint32_t* col_indices,
                       const bsmr_rphm_desc* desc, bsmr_blocked_stats* out, size_t out_size) {
    return bsmr_blocked_check_split(M, N, nnz, row_offsets, col_indices, desc, 0, out, out_size);
}

int bsmr_backward_attach_blocks_split(bsmr_backward* bw, const bsmr_rphm_desc* desc, uint32_t segment_blocks) {
    if (!bw || !desc || bw->blocked) return BSMR_ERR_INVALID_ARG;
    const uint32_t S = segment_blocks;
    const uint32_t M = bw->M, nnz = bw->nnz;
    constexpr uint32_t C = BSMR_BACKWARD_CHUNK;
    std::unique_ptr<BwBlocked> f;
    try {
        // the handle keeps S's CSR on the device only; its host copy for the check comes back from there
        std::vector<uint32_t> ro((size_t)M + 1u), ci(nnz);
        BSMR_HIP(hipSetDevice(bw->device));
        BSMR_HIP(hipMemcpy(ro.data(), bw->rowOffsets, ro.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
        if (nnz) BSMR_HIP(hipMemcpy(ci.data(), bw->colIndices, (size_t)nnz * sizeof(uint32_t), hipMemcpyDeviceToHost));
        BlockedHost h;
        if (int st = blockedCheck(M, bw->N, nnz, ro.data(), ci.data(), desc, S, h)) return st;

        const uint32_t P = desc->num_row_panels, rowsIn = desc->num_nonzero_rows;
        const uint32_t* bo = desc->block_offsets;
        std::vector<bsmr::BlkPanel> panels;
        std::vector<bsmr::BlkSegment> segs;          // S >= 1 only
        std::vector<bsmr::BlkSplit> splitPanels;
        uint32_t partials = 0;                       // at most one per block
        std::vector<uint32_t> panelRows, stageRow(M, bsmr::kBlkNull);   // stageRow[r]: staging row of r, or none
        for (uint32_t p = 0; p < P; ++p) {
            if (bo[p + 1] == bo[p]) continue;
            const uint32_t q = (uint32_t)panels.size();
            const uint32_t nb = bo[p + 1] - bo[p];
            panels.push_back({bo[p], nb});
            if (S && nb > S) {
                const uint32_t count = (uint32_t)segmentsOf(nb, S);
                splitPanels.push_back({q, partials, count});
                for (uint32_t k = 0, first = bo[p]; k < count; ++k, first += S)
                    segs.push_back({first, std::min(S, bo[p + 1] - first), q, partials++});
            } else if (S) {
                segs.push_back({bo[p], nb, q, bsmr::kBlkNull});
            }
            for (uint32_t i = 0; i < 16; ++i) {
                const uint32_t r = 16u * p + i < rowsIn ? desc->reordered_rows[16u * p + i] : bsmr::kBlkNull;
                panelRows.push_back(r);
                if (r != bsmr::kBlkNull) stageRow[r] = 16u * q + i;
            }
        }
        const uint64_t blocks = bo[P];
        std::vector<bsmr::u32x4> cells(64u * blocks), cols(4u * blocks);
        for (uint64_t b = 0; b < blocks; ++b) {
            const uint32_t* cell = desc->block_values + 256u * b;
            const uint32_t* col = desc->dense_cols + 16u * b;
            for (uint32_t l = 0; l < 64; ++l)
                for (uint32_t s = 0; s < 4; ++s) cells[64u * b + l][s] = cell[16u * (l & 15u) + 4u * s + (l >> 4)];
            for (uint32_t k = 0; k < 4; ++k)
                for (uint32_t s = 0; s < 4; ++s) cols[4u * b + k][s] = col[4u * s + k];
        }
        std::vector<uint32_t> resCols, resIdx;
        resCols.reserve(h.stats.residue_entries);
        resIdx.reserve(h.stats.residue_entries);
        for (uint32_t t = 0; t < nnz; ++t)
            if (!h.inBlock[t]) {
                resCols.push_back(ci[t]);
                resIdx.push_back(t);
            }
        // the schedule: the panels' rows in their order, then the rows in no panel
        std::vector<uint32_t> order(desc->reordered_rows, desc->reordered_rows + rowsIn);
        {
            std::vector<uint8_t> listed(M, 0);
            for (uint32_t r : order) listed[r] = 1;
            for (uint32_t r = 0; r < M; ++r)
                if (!listed[r]) order.push_back(r);
        }
        std::vector<bsmr::BwItem> items[2];
        std::vector<bsmr::BwSplit> splits[2];
        uint64_t slots = 0;
        for (uint32_t r : order) {
            const uint32_t b = h.resOffsets[r], e = h.resOffsets[r + 1];
            const int list = stageRow[r] != bsmr::kBlkNull;
            const uint32_t dest = list ? stageRow[r] : r;
            if (e - b <= C) {
                items[list].push_back({dest, b, e, bsmr::kBwDirect});
                continue;
            }
            const uint32_t chunks = (e - b + C - 1u) / C;
            splits[list].push_back({dest, (uint32_t)slots, chunks, 0});
            for (uint32_t k = 0, t = b; t < e; ++k, t += C) items[list].push_back({dest, t, std::min(e, t + C), (uint32_t)slots + k});
            slots += chunks;
        }
        if (slots > 0xFFFFFFFFull || items[0].size() > 0xFFFFFFFFull || items[1].size() > 0xFFFFFFFFull)
            return BSMR_ERR_INVALID_ARG;

        f.reset(new BwBlocked());
        f->stats = h.stats;
        f->numPanels = (uint32_t)panels.size();
        f->numSlots = (uint32_t)slots;
        f->segmentBlocks = S;
        f->numSegs = (uint32_t)segs.size();
        f->numSplitPanels = (uint32_t)splitPanels.size();
        f->numPartials = partials;
        uint64_t& bytes = f->stats.device_index_bytes;
        if (int st = upload(f->panels, panels, bytes)) return st;
        if (int st = upload(f->panelRows, panelRows, bytes)) return st;
        if (int st = upload(f->cells, cells, bytes)) return st;
        if (int st = upload(f->cols, cols, bytes)) return st;
        if (int st = upload(f->zeros, std::vector<float>(4, 0.f), bytes)) return st;
        if (int st = upload(f->resCols, resCols, bytes)) return st;
        if (int st = upload(f->resIdx, resIdx, bytes)) return st;
        if (int st = upload(f->segs, segs, bytes)) return st;
        if (int st = upload(f->splitPanels, splitPanels, bytes)) return st;
        for (int l = 0; l < 2; ++l) {
            if (int st = upload(f->items[l], items[l], bytes)) return st;
            if (int st = upload(f->splits[l], splits[l], bytes)) return st;
            f->numItems[l] = (uint32_t)items[l].size();
            f->numSplits[l] = (uint32_t)splits[l].size();
        }
    } catch (const std::bad_alloc&) {
        return BSMR_ERR_OOM;
    }
    bw->blocked = std::move(f);
    return BSMR_OK;
}

int bsmr_backward_attach_blocks(bsmr_backward* bw, const bsmr_rphm_desc* desc) {
    return bsmr_backward_attach_blocks_split(bw, desc, 0);
}

int bsmr_backward_get_blocked_stats(const bsmr_backward* bw, bsmr_blocked_stats* out, size_t out_size) {
    if (!bw || !out) return BSMR_ERR_INVALID_ARG;
    if (!bw->blocked) return BSMR_ERR_BAD_PLAN;
    memcpy(out, &bw->blocked->stats, std::min(out_size, sizeof(bsmr_blocked_stats)));
    return BSMR_OK;
}

int bsmr_spmm_blocked(bsmr_backward* bw, uint32_t K, const float* v_dev, const float* X_dev, float* Y_dev,
                      uint32_t num_batches, void* stream) {
    if (int st = checkBlockedCall(bw, K, true, num_batches, v_dev, X_dev, Y_dev)) return st;
    if (num_batches == 0) return BSMR_OK;
    BSMR_HIP(hipSetDevice(bw->device));
    if (int st = growWork(bw, workFloatsFor(bw, K, num_batches, false))) return st;
    return runBlocked(bw, K, v_dev, X_dev, Y_dev, num_batches, BSMR_COMPUTE_F32, static_cast<hipStream_t>(stream));
}

int bsmr_spmm_blocked_16(bsmr_backward* bw, uint32_t K, const float* v_dev, const void* X16_dev, void* Y16_dev,
                         uint32_t num_batches, int compute_mode, void* stream) {
    if (int st = checkBlockedCall(bw, K, is16(compute_mode), num_batches, v_dev, X16_dev, Y16_dev)) return st;
    if (num_batches == 0) return BSMR_OK;
    BSMR_HIP(hipSetDevice(bw->device));
    if (int st = growWork(bw, workFloatsFor(bw, K, num_batches, false))) return st;
    return runBlocked(bw, K, v_dev, X16_dev, Y16_dev, num_batches, compute_mode, static_cast<hipStream_t>(stream));
}

}  // extern "C"
