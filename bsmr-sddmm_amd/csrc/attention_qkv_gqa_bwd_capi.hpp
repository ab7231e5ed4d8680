// One-pass backward of sparse attention with grouped key/value heads (include/bsmr_hip.h "One-pass backward of sparse
// attention with grouped key/value heads"): the checks of bsmr_sparse_attention_qkv_backward_16 in its order with those of
// bsmr_sparse_attention_qkv_gqa_16 on kv_group, the workspace, D from csrc/attention_qkv_bwd_capi.hpp's launchQkvBwdRowDot
// and the launches of csrc/attention_qkv_gqa_bwd_kernels.hpp, a translation unit of their own (csrc/attention_qkv_gqa_bwd.hip).
//
// Workspace of a call with (K, Kv, b = num_batches, g = kv_group), in floats, from the start of the handle's workspace: the
// row partials [b][slots0][K], the column partials [b / g][slots1][K + Kv], then D [b][M].  K and Kv are multiples of 32, so
// every partial row starts on 16 bytes whatever M is.  It is never more than the ungrouped call's for b batches:
// bsmr_sparse_attention_qkv_backward_reserve(K, Kv, b) covers it.
// Included at the end of bsmr_capi.hip, after attention_qkv_bwd_capi.hpp (qkvBwdDim, runAttentionQkvBwd, launchQkvBwdRowDot).
#pragma once

#include "attention_qkv_launch.hpp"

extern "C" {

int bsmr_sparse_attention_qkv_gqa_backward_16(bsmr_backward* bw, uint32_t K, uint32_t Kv, float scale, const void* Q16_dev,
                                              const void* Kt16_dev, const void* V16_dev, const void* O16_dev,
                                              const void* dO16_dev, const float* m_dev, const float* s_dev, void* dQ16_dev,
                                              void* dKt16_dev, void* dV16_dev, uint32_t num_batches, uint32_t kv_group,
                                              int compute_mode, void* stream) {
    if (!bw || !std::isfinite(scale)) return BSMR_ERR_INVALID_ARG;
    if (kv_group == 0 || num_batches % kv_group != 0) return BSMR_ERR_INVALID_ARG;
    if (!qkvBwdDim(K) || !qkvBwdDim(Kv)) return BSMR_ERR_UNSUPPORTED_K;
    if (int st = checkAttentionCall(bw, Kv, scale, true, compute_mode, num_batches,
                                    {Q16_dev, Kt16_dev, V16_dev, O16_dev, dO16_dev}, {m_dev, s_dev}, {}))
        return st;
    if (!aligned16(dQ16_dev) || !aligned16(dKt16_dev) || !aligned16(dV16_dev)) return BSMR_ERR_INVALID_ARG;
    if (num_batches == 0 || (!dQ16_dev && !dKt16_dev && !dV16_dev)) return BSMR_OK;
    BSMR_HIP(hipSetDevice(bw->device));
    const uint16_t *Q = static_cast<const uint16_t*>(Q16_dev), *Kt = static_cast<const uint16_t*>(Kt16_dev);
    const uint16_t *V = static_cast<const uint16_t*>(V16_dev), *O = static_cast<const uint16_t*>(O16_dev);
    const uint16_t* dO = static_cast<const uint16_t*>(dO16_dev);
    uint16_t *dQ = static_cast<uint16_t*>(dQ16_dev), *dKt = static_cast<uint16_t*>(dKt16_dev);
    uint16_t* dV = static_cast<uint16_t*>(dV16_dev);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (kv_group == 1) return runAttentionQkvBwd(bw, K, Kv, scale, Q, Kt, V, O, dO, m_dev, s_dev, dQ, dKt, dV, num_batches, compute_mode, s);
    const uint64_t rowFloats = (uint64_t)bw->numSlots[0] * K * num_batches;
    const uint64_t colFloats = (uint64_t)bw->numSlots[1] * ((uint64_t)K + Kv) * (num_batches / kv_group);
    if (int st = growWork(bw, rowFloats + colFloats + (uint64_t)bw->M * num_batches)) return st;
    float* rowPart = bw->work;
    float* colPart = rowPart + rowFloats;
    float* D = colPart + colFloats;
    if (int st = launchQkvBwdRowDot(bw, O, dO, D, Kv, num_batches, compute_mode, s)) return st;
    const BsmrAttnBwdLists rowLists{bw->items[0].get(), bw->numItems[0], bw->splits[0].get(), bw->numSplits[0], bw->colIndices,
                                    bw->numSlots[0]};
    const BsmrAttnBwdLists colLists{bw->items[1].get(), bw->numItems[1], bw->splits[1].get(), bw->numSplits[1], bw->cscRows,
                                    bw->numSlots[1]};
    BSMR_HIP(bsmrLaunchAttnQkvGqaBwd(rowLists, colLists, scale, Q, Kt, V, dO, m_dev, s_dev, D, dQ, dKt, dV, rowPart, colPart, K, Kv,
                                     bw->M, bw->N, num_batches, kv_group, compute_mode == BSMR_COMPUTE_BF16, s));
    return BSMR_OK;
}

}  // extern "C"
