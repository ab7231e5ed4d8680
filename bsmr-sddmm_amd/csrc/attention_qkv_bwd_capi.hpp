// One-pass backward of sparse attention (include/bsmr_hip.h "One-pass backward of sparse attention"): the checks, the
// workspace and the launches of csrc/attention_qkv_bwd_kernels.hpp on the SDDMM backward's per-pattern handle - its row
// lists, its column lists (cscRows alone: no value array is read, so cscToCsr is not needed) and both chunk tables.
//
// Workspace of a call with (K, Kv, num_batches), in floats, from the start of the handle's workspace: the row partials
// [b][slots0][K], the column partials [b][slots1][K + Kv], then D [b][M] - b (M + slots0 K + slots1 (K + Kv)) in all,
// nothing of size nnz.  D lies last so that every partial row starts on 16 bytes whatever M is.  The offsets depend on
// (K, Kv, num_batches) alone.
// The kernels and their launches are a translation unit of their own, csrc/attention_qkv_bwd.hip; D comes from attnRowDot
// of this unit (csrc/attention_kernels.hpp).  Included at the end of bsmr_capi.hip, after attention_qkv_kv_capi.hpp.
#pragma once

#include "attention_qkv_launch.hpp"

namespace {

constexpr uint32_t kQkvBwdMaxK = 256;   // the column side holds 8 (K + Kv) / 32 fp32 accumulators per lane

bool qkvBwdDim(uint32_t k) { return k != 0 && (k & 31u) == 0 && k <= kQkvBwdMaxK; }

uint64_t qkvBwdPartFloats(const bsmr_backward* bw, uint32_t K, uint32_t Kv, uint32_t nb) {
    return ((uint64_t)bw->numSlots[0] * K + (uint64_t)bw->numSlots[1] * ((uint64_t)K + Kv)) * nb;
}

uint64_t qkvBwdWorkFloats(const bsmr_backward* bw, uint32_t K, uint32_t Kv, uint32_t nb) {
    return qkvBwdPartFloats(bw, K, Kv, nb) + (uint64_t)bw->M * nb;
}

// D [nb][M] = dO_r . O_r of every row, by attnRowDot; the grouped backward (attention_qkv_gqa_bwd_capi.hpp) starts with it too
int launchQkvBwdRowDot(const bsmr_backward* bw, const uint16_t* O, const uint16_t* dO, float* D, uint32_t Kv, uint32_t nb, int mode,
                       hipStream_t s) {
    const uint64_t rows = (uint64_t)bw->M * nb;
    if (bw->nnz && rows) {   // (without entries no kernel reads D, and O / dO may be NULL)
        const dim3 dgrid((uint32_t)((rows + 7u) / 8u));
        withMode(mode, [&](auto MODE) { hipLaunchKernelGGL(bsmr::attnRowDot<MODE()>, dgrid, dim3(256), 0, s, O, dO, D, rows, Kv); });
        BSMR_HIP(hipGetLastError());
    }
    return BSMR_OK;
}

int runAttentionQkvBwd(bsmr_backward* bw, uint32_t K, uint32_t Kv, float scale, const uint16_t* Q, const uint16_t* Kt,
                       const uint16_t* V, const uint16_t* O, const uint16_t* dO, const float* m, const float* sIn, uint16_t* dQ,
                       uint16_t* dKt, uint16_t* dV, uint32_t nb, int mode, hipStream_t s) {
    if (int st = growWork(bw, qkvBwdWorkFloats(bw, K, Kv, nb))) return st;
    float* rowPart = bw->work;
    float* colPart = rowPart + (uint64_t)bw->numSlots[0] * K * nb;
    float* D = bw->work + qkvBwdPartFloats(bw, K, Kv, nb);
    if (int st = launchQkvBwdRowDot(bw, O, dO, D, Kv, nb, mode, s)) return st;
    const BsmrAttnBwdLists rowLists{bw->items[0].get(), bw->numItems[0], bw->splits[0].get(), bw->numSplits[0], bw->colIndices,
                                    bw->numSlots[0]};
    const BsmrAttnBwdLists colLists{bw->items[1].get(), bw->numItems[1], bw->splits[1].get(), bw->numSplits[1], bw->cscRows,
                                    bw->numSlots[1]};
    BSMR_HIP(bsmrLaunchAttnQkvBwd(rowLists, colLists, scale, Q, Kt, V, dO, m, sIn, D, dQ, dKt, dV, rowPart, colPart, K, Kv, bw->M,
                                  bw->N, nb, mode == BSMR_COMPUTE_BF16, s));
    return BSMR_OK;
}

}  // namespace

extern "C" {

int bsmr_sparse_attention_qkv_backward_reserve(bsmr_backward* bw, uint32_t K, uint32_t Kv, uint32_t num_batches) {
    if (!bw) return BSMR_ERR_INVALID_ARG;
    if (!qkvBwdDim(K) || !qkvBwdDim(Kv)) return BSMR_ERR_UNSUPPORTED_K;
    if (num_batches > 65535u) return BSMR_ERR_INVALID_ARG;
    BSMR_HIP(hipSetDevice(bw->device));
    return growWork(bw, qkvBwdWorkFloats(bw, K, Kv, std::max(num_batches, 1u)));
}

int bsmr_sparse_attention_qkv_backward_16(bsmr_backward* bw, uint32_t K, uint32_t Kv, float scale, const void* Q16_dev,
                                          const void* Kt16_dev, const void* V16_dev, const void* O16_dev, const void* dO16_dev,
                                          const float* m_dev, const float* s_dev, void* dQ16_dev, void* dKt16_dev,
                                          void* dV16_dev, uint32_t num_batches, int compute_mode, void* stream) {
    if (!bw || !std::isfinite(scale)) return BSMR_ERR_INVALID_ARG;
    if (!qkvBwdDim(K) || !qkvBwdDim(Kv)) return BSMR_ERR_UNSUPPORTED_K;   // this call's limit: 256, not the forward's 512
    // (the order of bsmr_sparse_attention_qkv_16 from here on: compute_mode, the batches, then the pointers)
    if (int st = checkAttentionCall(bw, Kv, scale, true, compute_mode, num_batches,
                                    {Q16_dev, Kt16_dev, V16_dev, O16_dev, dO16_dev}, {m_dev, s_dev}, {}))
        return st;
    if (!aligned16(dQ16_dev) || !aligned16(dKt16_dev) || !aligned16(dV16_dev)) return BSMR_ERR_INVALID_ARG;
    if (num_batches == 0 || (!dQ16_dev && !dKt16_dev && !dV16_dev)) return BSMR_OK;
    BSMR_HIP(hipSetDevice(bw->device));
    return runAttentionQkvBwd(bw, K, Kv, scale, static_cast<const uint16_t*>(Q16_dev), static_cast<const uint16_t*>(Kt16_dev),
                              static_cast<const uint16_t*>(V16_dev), static_cast<const uint16_t*>(O16_dev),
                              static_cast<const uint16_t*>(dO16_dev), m_dev, s_dev, static_cast<uint16_t*>(dQ16_dev),
                              static_cast<uint16_t*>(dKt16_dev), static_cast<uint16_t*>(dV16_dev), num_batches, compute_mode,
                              static_cast<hipStream_t>(stream));
}

}  // extern "C"
