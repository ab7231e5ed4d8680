// One-pass sparse attention over the RPHM's blocks (include/bsmr_hip.h "One-pass sparse attention over blocks"): the
// checks, the lists, the workspace and the launches of csrc/attention_qkv_blocked_kernels.hpp on a handle with attached
// blocks (bsmr_backward_attach_blocks[_split]).
//
// Three launches of a call:
//   1. attnQkv / attnQkvMerge on the blocked format's items[0] / splits[0] over resCols: the rows in no panel with blocks,
//      stored directly, as bsmr_sparse_attention_qkv_16 stores them;
//   2. attnQkv on BwAttnBlk::items: the residue of the rows of panels with blocks, every chunk to a partial slot;
//   3. attnQkvBlocks over the panels or segments, then attnQkvBlkMerge over BwAttnBlk::rows.
// Workspace of a call with (Kv, num_batches), in floats, from the start of the handle's workspace: attnQkv's partial rows
// [b][slots][Kv], s_c and m_c [b][slots] (slots = BwAttnBlk::numSlots), rounded up to 16 bytes; then the block partials
// [b][16 units][Kv], their s and their m [b][16 units].  The offsets depend on (Kv, num_batches) alone.
// Included at the end of bsmr_capi.hip, after attention_qkv_capi.hpp.
#pragma once

namespace {

// The lists of the call, built once per handle.  Host work and two uploads; the blocked statistics are not touched.
int ensureAttnBlk(bsmr_backward* bw) {
    BwBlocked& f = *bw->blocked;
    if (f.attn) return BSMR_OK;
    try {
        std::unique_ptr<BwAttnBlk> a(new BwAttnBlk());
        const uint32_t P = f.numPanels, units = f.segmentBlocks ? f.numSegs : P;
        if (units > 0x0FFFFFFFu) return BSMR_ERR_INVALID_ARG;   // 16 rows per unit, numbered in 32 bits
        // the units of panel q: unitFirst[q] ... + unitCount[q] - 1 (the segments of a panel are consecutive)
        std::vector<uint32_t> unitFirst(P), unitCount(P, 1u);
        for (uint32_t q = 0; q < P; ++q) unitFirst[q] = q;
        if (f.segmentBlocks)
            for (uint32_t k = 0; k < f.numSegs; ++k) {
                const uint32_t q = f.hostSegs[k].panel;
                if (k == 0 || f.hostSegs[k - 1u].panel != q) {
                    unitFirst[q] = k;
                    unitCount[q] = 0;
                }
                ++unitCount[q];
            }
        // items[1] holds the residue of these rows chunk by chunk, a row's chunks side by side, under its staging row
        std::vector<bsmr::BwItem> items;
        std::vector<uint32_t> resFirst(16ull * P, 0u), resCount(16ull * P, 0u);
        uint64_t slot = f.numSlots;
        for (const bsmr::BwItem& it : f.hostItems1) {
            if (it.begin == it.end) continue;   // a row without residue gets no item
            if (!resCount[it.dest]++) resFirst[it.dest] = (uint32_t)slot;
            items.push_back({f.hostPanelRows[it.dest], it.begin, it.end, (uint32_t)slot});
            ++slot;
        }
        if (slot >= bsmr::kBwDirect) return BSMR_ERR_INVALID_ARG;
        std::vector<BsmrAttnBlkRow> rows;
        for (uint32_t q = 0; q < P; ++q)
            for (uint32_t i = 0; i < 16; ++i) {
                const uint32_t r = f.hostPanelRows[16u * q + i];
                if (r != bsmr::kBlkNull) rows.push_back({r, resFirst[16u * q + i], resCount[16u * q + i], 16u * unitFirst[q] + i, unitCount[q]});
            }
        a->numItems = (uint32_t)items.size();
        a->numRows = (uint32_t)rows.size();
        a->numSlots = (uint32_t)slot;
        a->numUnits = units;
        uint64_t bytes = 0;
        BSMR_HIP(hipSetDevice(bw->device));
        if (int st = upload(a->items, items, bytes)) return st;
        if (int st = upload(a->rows, rows, bytes)) return st;
        f.attn = std::move(a);
    } catch (const std::bad_alloc&) {
        return BSMR_ERR_OOM;
    }
    return BSMR_OK;
}

// floats of attnQkv's partial area, a multiple of 4: the block partials behind it are read as float4
uint64_t qkvBlkResFloats(const BwAttnBlk& a, uint32_t Kv, uint32_t nb) { return ((uint64_t)a.numSlots * (Kv + 2u) * nb + 3u) & ~3ull; }

uint64_t qkvBlkWorkFloats(const BwAttnBlk& a, uint32_t Kv, uint32_t nb) {
    return qkvBlkResFloats(a, Kv, nb) + 16ull * a.numUnits * (Kv + 2u) * nb;
}

// handle, K / Kv, compute_mode, batches, attached blocks - what the call and the reserve share, in the header's order
int checkQkvBlocked(const bsmr_backward* bw, uint32_t K, uint32_t Kv, bool modeOk, uint32_t nb) {
    if (!bw) return BSMR_ERR_INVALID_ARG;
    if (!qkvDim(K) || !qkvDim(Kv)) return BSMR_ERR_UNSUPPORTED_K;
    if (!modeOk || nb > 65535u) return BSMR_ERR_INVALID_ARG;
    return bw->blocked ? BSMR_OK : BSMR_ERR_BAD_PLAN;
}

int runAttentionQkvBlocked(bsmr_backward* bw, uint32_t K, uint32_t Kv, float scale, const uint16_t* Q, const uint16_t* Kt,
                           const uint16_t* V, uint16_t* O, float* m, float* sOut, uint32_t nb, int mode, hipStream_t s) {
    if (int st = ensureAttnBlk(bw)) return st;
    const BwBlocked& f = *bw->blocked;
    const BwAttnBlk& a = *f.attn;
    if (int st = growWork(bw, qkvBlkWorkFloats(a, Kv, nb))) return st;
    const uint32_t slots = a.numSlots;
    const bool bf16 = mode == BSMR_COMPUTE_BF16;
    float* partial = bw->work;
    float* sPart = partial + (uint64_t)slots * Kv * nb;
    float* mPart = sPart + (uint64_t)slots * nb;
    float* bPart = partial + qkvBlkResFloats(a, Kv, nb);
    float* bs = bPart + 16ull * a.numUnits * Kv * nb;
    float* bm = bs + 16ull * a.numUnits * nb;
    BSMR_HIP(bsmrLaunchAttnQkv(f.items[0].get(), f.numItems[0], f.splits[0].get(), f.numSplits[0], f.resCols, scale, Q, Kt, V, O, m,
                               sOut, partial, sPart, mPart, K, Kv, bw->M, bw->N, slots, nb, bf16, s));
    BSMR_HIP(bsmrLaunchAttnQkv(a.items.get(), a.numItems, nullptr, 0, f.resCols, scale, Q, Kt, V, O, m, sOut, partial, sPart, mPart,
                               K, Kv, bw->M, bw->N, slots, nb, bf16, s));
    const void* units = f.segmentBlocks ? static_cast<const void*>(f.segs.get()) : static_cast<const void*>(f.panels.get());
    BSMR_HIP(bsmrLaunchAttnQkvBlocks(units, a.numUnits, f.segmentBlocks != 0, f.panelRows, f.cells.get(), f.cols.get(), f.zeros,
                                     a.rows.get(), a.numRows, scale, Q, Kt, V, O, m, sOut, partial, sPart, mPart, slots, bPart, bs,
                                     bm, K, Kv, bw->M, bw->N, nb, bf16, s));
    return BSMR_OK;
}

}  // namespace

extern "C" {

int bsmr_sparse_attention_qkv_blocked_reserve(bsmr_backward* bw, uint32_t K, uint32_t Kv, uint32_t num_batches) {
    if (int st = checkQkvBlocked(bw, K, Kv, true, num_batches)) return st;
    if (int st = ensureAttnBlk(bw)) return st;
    BSMR_HIP(hipSetDevice(bw->device));
    return growWork(bw, qkvBlkWorkFloats(*bw->blocked->attn, Kv, std::max(num_batches, 1u)));
}

int bsmr_sparse_attention_qkv_blocked_16(bsmr_backward* bw, uint32_t K, uint32_t Kv, float scale, const void* Q16_dev,
                                         const void* Kt16_dev, const void* V16_dev, void* O16_dev, float* m_dev, float* s_dev,
                                         uint32_t num_batches, int compute_mode, void* stream) {
    if (!bw || !std::isfinite(scale)) return BSMR_ERR_INVALID_ARG;
    if (int st = checkQkvBlocked(bw, K, Kv, is16(compute_mode), num_batches)) return st;
    if (int st = checkAttentionCall(bw, Kv, scale, true, compute_mode, num_batches, {Q16_dev, Kt16_dev, V16_dev}, {},
                                    {O16_dev, m_dev, s_dev}))
        return st;
    if (!aligned16(O16_dev) || !aligned4(m_dev) || !aligned4(s_dev)) return BSMR_ERR_INVALID_ARG;
    if (num_batches == 0) return BSMR_OK;
    BSMR_HIP(hipSetDevice(bw->device));
    return runAttentionQkvBlocked(bw, K, Kv, scale, static_cast<const uint16_t*>(Q16_dev), static_cast<const uint16_t*>(Kt16_dev),
                                  static_cast<const uint16_t*>(V16_dev), static_cast<uint16_t*>(O16_dev), m_dev, s_dev, num_batches,
                                  compute_mode, static_cast<hipStream_t>(stream));
}

}  // extern "C"
