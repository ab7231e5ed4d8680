// One-pass grouped-head sparse attention on the MFMA (include/bsmr_hip.h "One-pass grouped-head sparse attention on the
// MFMA"): the checks of bsmr_sparse_attention_qkv_gqa_16 in its order, its workspace (csrc/attention_qkv_capi.hpp: the
// partials are indexed by query head, same layout, same reserve call) and the launch of
// csrc/attention_qkv_gqa_mfma_kernels.hpp, a translation unit of its own (csrc/attention_qkv_gqa_mfma.hip).  Every
// kv_group >= 1 is served by the one kernel: there is no hand-off at kv_group = 1, so K and Kv end at 256 there too.
// Included at the end of bsmr_capi.hip, after attention_qkv_gqa_capi.hpp (kQkvGqaMaxK).
#pragma once

#include "attention_qkv_launch.hpp"

extern "C" {

int bsmr_sparse_attention_qkv_gqa_mfma_16(bsmr_backward* bw, uint32_t K, uint32_t Kv, float scale, const void* Q16_dev,
                                          const void* Kt16_dev, const void* V16_dev, void* O16_dev, float* m_dev, float* s_dev,
                                          uint32_t num_batches, uint32_t kv_group, int compute_mode, void* stream) {
    if (!bw || !std::isfinite(scale)) return BSMR_ERR_INVALID_ARG;
    if (kv_group == 0 || num_batches % kv_group != 0) return BSMR_ERR_INVALID_ARG;
    if (!qkvDim(K) || !qkvDim(Kv) || K > kQkvGqaMaxK || Kv > kQkvGqaMaxK) return BSMR_ERR_UNSUPPORTED_K;
    if (int st = checkAttentionCall(bw, Kv, scale, true, compute_mode, num_batches, {Q16_dev, Kt16_dev, V16_dev}, {},
                                    {O16_dev, m_dev, s_dev}))
        return st;
    if (!aligned16(O16_dev) || !aligned4(m_dev) || !aligned4(s_dev)) return BSMR_ERR_INVALID_ARG;
    if (num_batches == 0) return BSMR_OK;
    BSMR_HIP(hipSetDevice(bw->device));
    if (int st = growWork(bw, qkvWorkFloats(bw, Kv, num_batches))) return st;
    const uint32_t slots = bw->numSlots[0];
    float* partial = bw->work;
    float* sPart = bw->work + (uint64_t)slots * Kv * num_batches;
    float* mPart = sPart + (uint64_t)slots * num_batches;
    BSMR_HIP(bsmrLaunchAttnQkvGqaMfma(bw->items[0].get(), bw->numItems[0], bw->splits[0].get(), bw->numSplits[0], bw->colIndices,
                                      scale, static_cast<const uint16_t*>(Q16_dev), static_cast<const uint16_t*>(Kt16_dev),
                                      static_cast<const uint16_t*>(V16_dev), static_cast<uint16_t*>(O16_dev), m_dev, s_dev,
                                      partial, sPart, mPart, K, Kv, bw->M, bw->N, slots, num_batches, kv_group,
                                      compute_mode == BSMR_COMPUTE_BF16, static_cast<hipStream_t>(stream)));
    return BSMR_OK;
}

}  // extern "C"
